"""The DDPG head's entry points without a GPU: header, library and binding agree; the workspace follows its formula; every refusal
comes before any launch (fake addresses); the numpy restatements of tests/ddpg_util.py are what torch indexing and torch float64
autograd give; the learner case's kink filter stays under its cap; the stepped case (a whole update from distinct target networks)
stays under the cap at its fixed point, and every misreading of the update lies far from its float64 reference; DDPGLearner and the
bindings refuse on the host."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import actor_grad_util as U
import ddpg_util as D
import offpolicy_util as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bsx_ddpg_inputs", "bsx_ddpg_put_actions", "bsx_td_head_workspace_bytes", "bsx_td_head", "bsx_ddpg_action_grad")
ARG, ALIGN = -1, -2
A16, A4, A1 = 4096, 4096 + 4, 4096 + 1


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
    assert L.ABI_VERSION == 14 == lib.bsx_abi_version()
    for struct, fields in ((L.BsxDdpgBatch, ("obs", "obs_next", "act")), (L.BsxTdIo, ("q", "q_next", "rew", "done", "weight", "g_q", "g_pi", "td"))):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), hdr, flags=re.S).group(1)
        assert tuple(re.findall(r"(\w+);", body)) == fields == tuple(f for f, _ in struct._fields_)
    import deep_rl_battlespace_amd as pkg
    for name in ("DDPGLearner", "ddpg_inputs", "ddpg_put_actions", "td_head", "ddpg_action_grad", "td_head_workspace_bytes", "TD_STATS"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert len(pkg.TD_STATS) == 8


def test_the_workspace_is_64_bytes_per_workgroup_of_the_plan():
    lib, nb = _L().load(), ctypes.c_size_t()
    for B, nA in [s[:2] for s in D.SHAPES] + [(512, 2), (65536, 2), (16384, 16), ((1 << 31) - 1, 16)]:
        assert lib.bsx_td_head_workspace_bytes(B, nA, ctypes.byref(nb)) == 0
        assert nb.value == 64 * D.plan(B, nA)[2], (B, nA)
    # the larger shape is the first B at nA = 16 whose workgroups take two tiles; its merge goes round more than once
    B, nA = D.LARGE[:2]
    assert D.plan(B, nA)[1] == 2 and D.plan(B - 1, nA)[1] == 1 and D.plan(B, nA)[3] > 1
    assert all(D.plan(*s[:2])[1] == 1 for s in D.SHAPES[:-1])
    for B_, nA_ in ((0, 2), (1 << 31, 2), (10, 0), (10, 17)):
        assert lib.bsx_td_head_workspace_bytes(B_, nA_, ctypes.byref(nb)) == ARG
    assert lib.bsx_td_head_workspace_bytes(10, 2, None) == ARG


def test_every_entry_refuses_what_the_header_documents_before_any_launch():
    """Fake addresses only: every call is refused before anything reaches HIP."""
    L = _L()
    lib = L.load()
    shapes_bad = [dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=17), dict(Do=0), dict(Do=51), dict(k=2), dict(k=5), dict(central=2),
                  dict(central=-1), dict(nA=4, Do=14, k=4, central=1),                       # 4v4 central: 72 inputs
                  dict(nA=2, Do=30, k=4, central=1)]                                        # 68 inputs

    def inputs(B=100, nA=2, Do=8, k=4, central=1, batch=True, x_cur=A4, x_next=A4, x_pi=A4, **ptr):
        st = L.BsxDdpgBatch(**{f: ptr.get(f, A4) for f in ("obs", "obs_next", "act")})
        return lib.bsx_ddpg_inputs(ctypes.byref(st) if batch else None, B, nA, Do, k, central, x_cur, x_next, x_pi, None)

    def put(B=100, nA=2, Do=8, k=4, central=1, own_only=0, y4=A16, x=A4):
        return lib.bsx_ddpg_put_actions(y4, B, nA, Do, k, central, own_only, x, None)

    def grad(B=100, nA=2, Do=8, k=4, central=1, gx=A4, g_a4=A16):
        return lib.bsx_ddpg_action_grad(gx, B, nA, Do, k, central, g_a4, None)

    for call in (inputs, put, grad):
        for kw in shapes_bad:
            assert call(**kw) == ARG, (call.__name__, kw)
    for kw in (dict(batch=False), dict(obs=None), dict(obs_next=None), dict(act=None), dict(x_cur=None), dict(x_next=None), dict(x_pi=None)):
        assert inputs(**kw) == ARG, kw
    for kw in (dict(obs=A1), dict(obs_next=A1), dict(act=A1), dict(x_cur=A1), dict(x_next=A1), dict(x_pi=A1)):
        assert inputs(**kw) == ALIGN, kw
    assert inputs(obs=A1, k=5) == ARG                                                       # argument rules before alignment rules
    for kw in (dict(y4=None), dict(x=None), dict(own_only=2), dict(own_only=-1)):
        assert put(**kw) == ARG, kw
    assert put(y4=A4) == ALIGN and put(x=A1) == ALIGN and put(y4=A4, nA=17) == ARG
    for kw in (dict(gx=None), dict(g_a4=None)):
        assert grad(**kw) == ARG, kw
    assert grad(g_a4=A4) == ALIGN and grad(gx=A1) == ALIGN and grad(g_a4=A4, Do=0) == ARG

    fields = [f for f, _ in L.BsxTdIo._fields_]

    def td(B=100, nA=2, gamma=0.95, ws=A16, stats=A16, io=True, **ptr):
        st = L.BsxTdIo(**{f: ptr.get(f, None if f in ("weight", "td") else A16) for f in fields})
        return lib.bsx_td_head(ctypes.byref(st) if io else None, B, nA, gamma, ws, stats, None)

    nan = float("nan")
    for kw in [dict(io=False), dict(ws=None), dict(stats=None)] + [{f: None} for f in fields if f not in ("weight", "td")] + \
            [dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=nan), dict(gamma=float("inf")), dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=17)]:
        assert td(**kw) == ARG, kw
    for kw in [{f: A4} for f in ("g_q", "g_pi")] + [{f: A1} for f in ("q", "q_next", "rew", "weight", "td")] + [dict(ws=A4), dict(stats=A4)]:
        assert td(**kw) == ALIGN, kw
    for kw in (dict(g_q=A4, gamma=2.0), dict(ws=A4, B=0), dict(q=A1, rew=None)):
        assert td(**kw) == ARG, kw
    assert td(g_q=A4, done=A1, gamma=0.0) == ALIGN and td(g_q=A4, gamma=1.0) == ALIGN     # done at any byte; the ends of [0, 1] are in


@pytest.mark.parametrize("shape", D.SHAPES[:-1], ids=D.shape_id)
def test_the_copy_restatements_are_torch_cat_and_indexing(shape):
    B, nA, Do, k, central = shape
    Dc = D.width(nA, Do, k, central)
    obs, obs_next, act = D.batch_arrays(shape)
    g = np.random.default_rng(5)
    poison = [np.full((B, nA, Dc), np.nan, np.float32) for _ in range(3)]
    x_cur, x_next, x_pi = D.ref_inputs(obs, obs_next, act, central, *poison)
    to, oa = torch.from_numpy, (obs, act)
    if central:
        want = torch.cat([to(obs).reshape(B, 1, -1), to(act).reshape(B, 1, -1)], -1).expand(B, nA, Dc)
    else:
        want = torch.cat([to(o) for o in oa], -1)
    W = Dc - (nA * k if central else k)
    assert np.array_equal(x_cur, want.numpy())
    assert np.array_equal(x_pi[..., :W], x_cur[..., :W]) and np.array_equal(x_next[..., :W], D.join(obs_next, act, central)[..., :W])
    assert np.isnan(x_next[..., W:]).all() and (np.array_equal(x_pi[..., W:], x_cur[..., W:]) if central else np.isnan(x_pi[..., W:]).all())
    y4 = g.standard_normal((B, nA, 4)).astype(np.float32)
    every = D.ref_put_actions(y4, x_next, Do, k, central, False)
    assert np.array_equal(every, D.join(obs_next, y4[..., :k], central))                    # x_next: the target actors' joint action
    own = D.ref_put_actions(y4, x_pi, Do, k, central, True)
    for i in range(nA):                                                                     # x_pi: slot i replaced, the others replayed
        mixed = act.copy()
        mixed[:, i] = y4[:, i, :k]
        assert np.array_equal(own[:, i], D.join(obs, mixed, central)[:, i])
    gx = g.standard_normal((B, nA, Dc)).astype(np.float32)
    ga = D.ref_action_grad(gx, Do, k, central)
    for i in range(nA):
        c0 = nA * Do + i * k if central else Do
        assert np.array_equal(ga[:, i, :k], gx[:, i, c0:c0 + k])
    assert k == 4 or (not ga[..., 3].any() and not np.signbit(ga[..., 3]).any())


@pytest.mark.parametrize("weight", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_the_td_restatement_is_float64_autograd_of_the_two_losses(shape, weight):
    inp = D.td_inputs(*shape[:2])
    ref, t64 = D.HEAD.ref(inp, weight=weight), D.HEAD.autograd(inp, torch.float64, weight=weight)
    for k in D.HEAD.names:
        err = float(np.abs(ref[k] - t64[k]).max() / np.abs(t64[k]).max())
        assert err <= 1e-12, (k, err)
    assert ref["stats"][0] == t64["stats"][0] == inp["q"].numel() and ref["stats"][7] == 0.0
    for i in range(1, 7):
        assert abs(ref["stats"][i] - t64["stats"][i]) <= 1e-12 * max(abs(t64["stats"][i]), 1e-300), i
    assert not ref["g_q"][..., 1:].any() and not ref["g_pi"][..., 1:].any()
    # a finished row's target is its reward, whatever q_next holds; gamma = 0 likewise
    over = inp["done"].numpy() != 0
    assert np.array_equal(ref["td"][over], inp["rew"].double().numpy()[over])
    bad = dict(inp, q_next=torch.where(inp["done"] != 0, torch.tensor(float("nan")), inp["q_next"]))
    assert all(np.array_equal(D.HEAD.ref(bad, weight=weight)[k], ref[k]) for k in D.HEAD.names + ("stats",))
    assert np.array_equal(D.HEAD.ref(inp, gamma=0.0)["td"], inp["rew"].double().numpy())


@pytest.mark.parametrize("shape", D.KINK_SHAPES, ids=lambda s: "B%d-nA%d-Do%d-k%d" % s)
def test_the_kink_filter_of_the_learner_case_stays_under_the_cap(shape):
    """Row weights are 0 where, in float64, a pre-ReLU value of the critic at x_cur or x_pi or of the actor at obs lies within KINK of 0.
    Measured here over seeds 0 .. 2, own and central where central fits: between 1.0 % and 4.4 % of the elements."""
    B, nA, Do, k = shape
    for central in (0, 1):
        if central and D.width(nA, Do, k, 1) > 64:
            continue
        for seed in range(3):
            *_, w, share = D.learner_case((B, nA, Do, k, central), seed)
            print(shape, "central" if central else "own", "seed", seed, f"left out {100 * share:.2f} %")
            assert share < U.KINK_CAP and float((w == 0).double().mean()) == share


@pytest.mark.parametrize("shape", D.LEARNER_SHAPES, ids=D.shape_id)
def test_the_stepped_case_stays_under_the_cap_and_its_kink_filter_has_reached_its_fixed_point(shape):
    """stepped_case's row weights are 0 also where the STEPPED critic has a pre-ReLU value within KINK of 0 at x_pi; zeroing a row moves
    that critic, so the filter is repeated.  It closed within MAX_ROUNDS and under the cap (both conditions on the float64 reference:
    STEP_SEEDS), and at the end no row that still has a weight lies near a kink of the final stepped critic -- nor of the starting
    networks, whose filter (learner_case's) the weights started from."""
    B, nA, Do, k, central = shape
    c = D.stepped_case(shape)
    print(D.shape_id(shape), f"seed {c.seed}: left out {100 * c.share:.2f} % after {c.rounds} zeroing rounds")
    assert c.share < U.KINK_CAP and c.rounds <= O.MAX_ROUNDS and float((c.w == 0).double().mean()) == c.share
    obs, act, _, obs_next, _ = c.batch
    x_cur, _, x_pi = D.joins64(c.actor, obs, obs_next, act, central)
    stepped = c.ref["critic"]["net"]
    assert stepped.w1.dtype == torch.float64 and not torch.equal(stepped.w1, c.critic.w1.double())
    near = torch.zeros((B, nA), dtype=torch.bool)
    for net, x in ((stepped, x_pi), (c.critic, x_pi), (c.critic, x_cur), (c.actor, obs)):
        near |= (U.pre_relu64(net, x).abs() < U.KINK).any(-1).transpose(0, 1)
    assert not (near & (c.w != 0)).any()
    _, _, _, _, w0, _ = D.learner_case(shape, c.seed)
    assert bool(((c.w == 0) | (c.w == w0)).all()) and bool((w0[c.w != 0] != 0).all())      # rows were only ever zeroed
    # the reference's own step: the targets moved by tau towards the stepped networks, the moments are the first step's
    tau = float(np.float32(D.STEP_KW["tau"]))
    for net, start, target in ((c.ref["critic"], c.critic, c.tc), (c.ref["actor"], c.actor, c.ta)):
        for p, new, t_new, m in zip(D.PARAMS, net["p"], net["target"], net["m"]):
            t0 = getattr(target, p).detach().double().numpy()
            assert np.allclose(t_new, (1 - tau) * t0 + tau * new, rtol=0, atol=1e-15)
            assert np.abs(new - getattr(start, p).detach().double().numpy()).max() <= 1.0001 * max(D.STEP_KW["lr_critic"], D.STEP_KW["lr_actor"])
        assert 0.0 < net["coef"] <= 1.0 and net["norm"] > 0.0


@pytest.mark.parametrize("shape", D.LEARNER_SHAPES, ids=D.shape_id)
def test_every_wrong_reading_of_the_update_lies_far_from_the_reference(shape):
    """What the float64 test of the update on the GPU can tell apart, shown on the CPU in float64 alone: the critic's gradient with the
    live networks in place of the targets (both, the actor alone, the critic alone) and the actor's gradient at the unstepped critic
    each lie, in the mean over w1, w2, w3 and b3 each, at least 1000 x the float32 yardstick's mean error from the right gradient -- a
    condition (measured: 2e5 x and more), so a learner that made one of these mistakes cannot pass within the (2, 4) bars."""
    c = D.stepped_case(shape)
    assert not bool(c.batch[4].all())                             # some row is unfinished: the targets are read at all
    smallest = {}
    for name, (dist, yard) in D.wrong_variants(c, shape[4]).items():
        ratios = {p: dist[p] / yard[p] for p in D.SHARP}
        smallest[name] = min(ratios.values())
        assert all(yard[p] > 0.0 for p in D.SHARP) and min(ratios.values()) >= 1000.0, (name, ratios)
    print(D.shape_id(shape), "smallest wrong-variant ratio: " + ", ".join(f"{k} {v:.3g}" for k, v in smallest.items()))


def test_the_profile_records_the_stepped_cases_and_its_factors_are_the_rule_on_the_recorded_spread():
    """profiles/ddpg_float64.json: per shape the seed, the share left out and the rounds stepped_case gives; the factor exceptions are
    mlp_grad_util.factor_rule of the yardstick's recorded spread and nothing else; every recorded kernel ratio lies within its bars."""
    rec = json.load(open(D.PROFILE))["stepped"]
    assert rec["factors"] == D.stepped_exceptions(rec["spread"]) and set(rec["factors"]) <= {"*"}
    assert set(rec["cases"]) == set(rec["spread"]) == set(rec["kernel"]) == {D.shape_id(s) for s in D.LEARNER_SHAPES}
    for shape in D.LEARNER_SHAPES:
        c, r = D.stepped_case(shape), rec["cases"][D.shape_id(shape)]
        assert r["seed"] == c.seed == D.STEP_SEEDS.get(shape, 0) and r["zeroing_rounds"] == c.rounds
        assert abs(r["left_out_percent"] - 100 * c.share) <= 0.005 + 1e-9
        assert min(rec["sharpness"][D.shape_id(shape)].values()) >= 1000
        for name, (mean, mx) in rec["kernel"][D.shape_id(shape)].items():
            which, tensor = name.split(".")
            fm, fx = D.stepped_factor_of(shape, which)(tensor) if which in ("gc", "ga") else (D.FM, D.FX)
            assert mean <= fm and mx <= fx, (shape, name)


def test_the_maddpg_losses_of_the_reference_agree_with_the_by_hand_joins_in_float64():
    """maddpg_grads' central actor loss reads, for agent i, the replayed joint action with slot i replaced by pi_i(o_i): the joins the
    kernels make (ref_inputs + ref_put_actions), fed to the critic in float64, give the same loss gradient with respect to pi."""
    shape = (33, 3, 4, 3, 1)
    B, nA, Do, k, central = shape
    actor, critic = D.make_nets(nA, Do, k, central)
    obs, act, rew, obs_next, done = D.ring_rows(B, nA, Do, k)
    w = torch.ones((B, nA))
    _, ga = D.maddpg_grads(actor, critic, (obs, act, rew, obs_next, done), w, central, torch.float64)
    a64, c64 = D.R.to_float64(actor), D.R.to_float64(critic)
    pi = a64(obs.double())
    x_pi = torch.from_numpy(D.join(obs.double().numpy(), act.double().numpy(), central)).clone()
    x = x_pi.clone().requires_grad_()
    with torch.no_grad():
        pad = torch.cat([pi, torch.zeros((B, nA, 1), dtype=torch.float64)], -1).numpy()
        x.data.copy_(torch.from_numpy(D.ref_put_actions(pad, x_pi.numpy(), Do, k, central, True)))
    (-(c64(x, squash=False)[..., 0]).mean(0).sum()).backward()
    g_a = torch.from_numpy(D.ref_action_grad(x.grad.numpy(), Do, k, central)[..., :k])
    (pi * g_a).sum().backward()
    for p in D.PARAMS:
        got, want = getattr(a64, p).grad.numpy(), ga[p]
        assert float(np.abs(got - want).max()) <= 1e-12 * max(float(np.abs(want).max()), 1e-300), p


def test_the_bindings_and_the_learner_refuse_on_the_host():
    from deep_rl_battlespace_amd import learner as L
    with pytest.raises(ValueError, match="4v4 central is 72"):
        L._critic_width(4, 14, 4, True)
    assert L._critic_width(4, 14, 4, False) == 18 and L._critic_width(3, 11, 4, True) == 45
    with pytest.raises(ValueError, match="3 or 4 action columns"):
        L._critic_width(2, 8, 2, True)
    with pytest.raises(ValueError, match="GPU"):
        L.td_head(*(torch.zeros((4, 2)) for _ in range(3)), torch.zeros((4, 2), dtype=torch.uint8), 0.9)
    with pytest.raises(ValueError, match="GPU"):
        L.ddpg_inputs(torch.zeros((4, 2, 5)), torch.zeros((4, 2, 5)), torch.zeros((4, 2, 4)))
    with pytest.raises(ValueError, match="DeviceReplayBuffer"):
        L.DDPGLearner(object(), None)
