"""The SAC entry points without a GPU: header, library and binding agree and the ABI version stays; the workspaces follow their
formulas; every refusal the header documents comes before any launch (fake addresses); the bindings and SACLearner's constructor refuse
on the host; the numpy restatements of tests/sac_util.py are what torch float64 autograd of L_critic, L_pi and L_alpha gives; the
whole-update case stays under the kink cap at its fixed point, every misreading of the update lies far from its float64 reference, and
profiles/sac_float64.json records what the case gives."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ddpg_util as D
import offpolicy_util as O
import sac_util as S
import td3_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bsx_sac_sample_actions", "bsx_sac_head_workspace_bytes", "bsx_sac_head", "bsx_sac_policy_seed", "bsx_sac_policy_grad_workspace_bytes",
           "bsx_sac_policy_grad")
HEAD_FIELDS = ("q1", "q2", "q1_next", "q2_next", "logp_next", "rew", "done", "weight", "log_alpha", "g_q1", "g_q2", "td")
PI_FIELDS = ("gx1", "gx2", "z", "logp", "q1_pi", "q2_pi", "weight", "log_std", "log_alpha", "g_a4", "g_log_std", "g_log_alpha", "alpha_m", "alpha_v",
             "hyper", "step")
ARG, ALIGN = -1, -2
A16, A8, A4, A1 = 4096, 4096 + 8, 4096 + 4, 4096 + 1
NAN, INF = float("nan"), float("inf")


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
    assert L.ABI_VERSION == 14 == lib.bsx_abi_version() and "#define BSX_ABI_VERSION 14" in hdr
    for struct, fields, cls in (("BsxSacIo", HEAD_FIELDS, L.BsxSacIo), ("BsxSacPolicyIo", PI_FIELDS, L.BsxSacPolicyIo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        assert tuple(re.findall(r"(\w+);", body)) == fields == tuple(f for f, _ in cls._fields_), struct
    import deep_rl_battlespace_amd as pkg
    for name in ("SACLearner", "sac_sample_actions", "sac_head", "sac_head_workspace_bytes", "sac_policy_seed", "sac_policy_grad",
                 "sac_policy_grad_workspace_bytes", "SacHead", "SacPolicyGrad", "SAC_STATS", "SAC_PI_STATS"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pkg.learner, name), name
    assert pkg.SAC_STATS == pkg.TD3_STATS and issubclass(pkg.SACLearner, pkg.DDPGLearner)
    assert pkg.SAC_PI_STATS == ("n", "actor_loss", "q_pi", "logp", "alpha", "weight", "picked_1", "reserved")
    assert "#define BSX_SAC_SALT 0x60000000u" in hdr and S.SALT == L.SAC_SALT == 0x60000000
    assert S.SALT not in S.OTHER_SALTS and len(set(S.OTHER_SALTS)) == 5
    doc = pkg.SACLearner.__doc__
    assert "tanh-squash" in doc and "six head outputs" in doc and "target_actor" in doc and "never read or stepped" in doc
    assert "A SAC update:" in pkg.learner.__doc__


def _pi_plan(B, nA):
    S_ = (256 // nA) * nA
    tiles = -(-B * nA // S_)
    J = -(-tiles // 1024)
    return tiles, J, -(-tiles // J)


def test_the_workspaces_follow_their_formulas():
    lib, nb, nb0 = _L().load(), ctypes.c_size_t(), ctypes.c_size_t()
    shapes = S.HEAD_SHAPES + ((512, 2), (65536, 2), (16384, 16), (129, 3), (100000, 7), ((1 << 31) - 1, 16))
    for B, nA in shapes:
        assert lib.bsx_sac_head_workspace_bytes(B, nA, ctypes.byref(nb)) == 0 == lib.bsx_td3_head_workspace_bytes(B, nA, ctypes.byref(nb0))
        assert nb.value == 64 * D.plan(B, nA)[2] == nb0.value, (B, nA)
        assert lib.bsx_sac_policy_grad_workspace_bytes(B, nA, ctypes.byref(nb)) == 0
        assert nb.value == 8 * (8 + 5 * nA) * _pi_plan(B, nA)[2], (B, nA)
    assert _pi_plan(16385, 16)[1] == 2 and _pi_plan(130, 16)[1] == 1 and _pi_plan(100000, 7)[0] == -(-700000 // 252)
    for entry in (lib.bsx_sac_head_workspace_bytes, lib.bsx_sac_policy_grad_workspace_bytes):
        for B_, nA_ in ((0, 2), (1 << 31, 2), (10, 0), (10, 17)):
            assert entry(B_, nA_, ctypes.byref(nb)) == ARG
        assert entry(10, 2, None) == ARG


def test_every_entry_refuses_what_the_header_documents_before_any_launch():
    """Fake addresses only: every call is refused before anything reaches HIP."""
    L = _L()
    lib = L.load()
    shapes = [dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=17), dict(Do=0), dict(Do=51), dict(k=2), dict(k=4), dict(k=5), dict(central=2),
              dict(central=-1), dict(nA=4, Do=14, central=1), dict(nA=2, Do=30, central=1)]               # Dc = 68 and 66 > 64

    def sample(B=100, nA=2, Do=8, k=3, central=1, own_only=0, y4=A16, ls=A4, x=A4, logp=A4, z_out=None, seq_base=None, z=None):
        return lib.bsx_sac_sample_actions(y4, ls, B, nA, Do, k, central, own_only, 1, 2, seq_base, z, x, logp, z_out, None)

    for kw in shapes + [dict(y4=None), dict(ls=None), dict(x=None), dict(logp=None), dict(own_only=2), dict(own_only=-1)]:
        assert sample(**kw) == ARG, kw
    for kw in (dict(y4=A4), dict(y4=A8), dict(z=A4), dict(z=A8), dict(z_out=A4), dict(z_out=A8), dict(x=A1), dict(ls=A1), dict(logp=A1),
               dict(seq_base=A4), dict(seq_base=A1)):
        assert sample(**kw) == ALIGN, kw
    for kw in (dict(y4=A4, k=4), dict(x=A1, own_only=2), dict(z=A4, logp=None), dict(seq_base=A4, nA=17)):   # argument rules before alignment rules
        assert sample(**kw) == ARG, kw

    def head(B=100, nA=2, gamma=0.95, ws=A16, stats=A16, io=True, **ptr):
        st = L.BsxSacIo(**{f: ptr.get(f, None if f in ("weight", "td") else A16) for f in HEAD_FIELDS})
        return lib.bsx_sac_head(ctypes.byref(st) if io else None, B, nA, gamma, ws, stats, None)

    for kw in [dict(io=False), dict(ws=None), dict(stats=None)] + [{f: None} for f in HEAD_FIELDS if f not in ("weight", "td")] + \
            [dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=NAN), dict(gamma=INF), dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=17)]:
        assert head(**kw) == ARG, kw
    for kw in [{f: A4} for f in ("g_q1", "g_q2")] + [{f: A1} for f in ("q1", "q2", "q1_next", "q2_next", "logp_next", "rew", "weight", "log_alpha", "td")] + \
            [dict(ws=A4), dict(stats=A4)]:
        assert head(**kw) == ALIGN, kw
    for kw in (dict(g_q2=A4, gamma=2.0), dict(ws=A4, B=0), dict(q2=A1, logp_next=None)):
        assert head(**kw) == ARG, kw
    assert head(g_q2=A4, done=A1, gamma=0.0) == ALIGN and head(g_q1=A4, gamma=1.0) == ALIGN   # done at any byte; the ends of [0, 1] are in

    def seed(B=100, nA=2, q1=A4, q2=A4, w=None, g1=A16, g2=A16):
        return lib.bsx_sac_policy_seed(q1, q2, w, B, nA, g1, g2, None)

    for kw in (dict(q1=None), dict(q2=None), dict(g1=None), dict(g2=None), dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=17)):
        assert seed(**kw) == ARG, kw
    for kw in (dict(g1=A4), dict(g2=A8), dict(q1=A1), dict(q2=A1), dict(w=A1)):
        assert seed(**kw) == ALIGN, kw
    assert seed(g1=A4, nA=17) == ARG

    optional = ("weight", "alpha_m", "alpha_v", "hyper", "step")

    def grad(B=100, nA=2, Do=8, k=3, central=1, te=-3.0, ws=A16, stats=A16, io=True, **ptr):
        st = L.BsxSacPolicyIo(**{f: ptr.get(f, None if f in optional else A16) for f in PI_FIELDS})
        return lib.bsx_sac_policy_grad(ctypes.byref(st) if io else None, B, nA, Do, k, central, te, ws, stats, None)

    adam = dict(alpha_m=A4, alpha_v=A4, hyper=A4, step=A8)
    for kw in [dict(io=False), dict(ws=None), dict(stats=None)] + [{f: None} for f in PI_FIELDS if f not in optional] + shapes + \
            [dict(te=NAN), dict(te=INF), dict(te=-INF)] + [{k_: v for k_, v in adam.items() if k_ != drop} for drop in adam] + [dict(step=A8)]:
        assert grad(**kw) == ARG, kw
    for kw in [{f: A4} for f in ("z", "g_a4")] + [{f: A1} for f in ("gx1", "gx2", "logp", "q1_pi", "q2_pi", "weight", "log_std", "log_alpha", "g_log_std",
                                                                 "g_log_alpha")] + [dict(ws=A4), dict(stats=A4), dict(adam, step=A4),
                                                                                    dict(adam, alpha_m=A1), dict(adam, hyper=A1)]:
        assert grad(**kw) == ALIGN, kw
    for kw in (dict(z=A4, k=4), dict(ws=A4, te=NAN), dict(g_a4=A4, alpha_m=A4)):
        assert grad(**kw) == ARG, kw


def test_the_bindings_and_the_learners_constructor_refuse_on_the_host():
    from deep_rl_battlespace_amd import learner as L
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    from deep_rl_battlespace_amd.rollout import StackedActor
    z = torch.zeros((4, 2))
    with pytest.raises(ValueError, match="GPU"):
        L.sac_head(z, z, z, z, z, z, torch.zeros((4, 2), dtype=torch.uint8), torch.zeros(2), 0.9)
    with pytest.raises(ValueError, match="GPU"):
        L.sac_sample_actions(torch.zeros((4, 2, 4)), torch.zeros((2, 3)), torch.zeros((4, 2, 22)), 8, 3)
    with pytest.raises(ValueError, match="n_actions must be 3"):
        L.sac_sample_actions(torch.zeros((4, 2, 4)), torch.zeros((2, 3)), torch.zeros((4, 2, 24)), 8, 4)
    with pytest.raises(ValueError, match="GPU"):
        L.sac_policy_seed(z, z)
    with pytest.raises(ValueError, match="GPU"):
        L.sac_policy_grad(torch.zeros((4, 2, 22)), torch.zeros((4, 2, 22)), torch.zeros((4, 2, 4)), z, z, z, torch.zeros((2, 3)), torch.zeros(2), 8)
    with pytest.raises(ValueError, match="n_actions must be 3"):
        L.sac_policy_grad(torch.zeros((4, 2, 24)), torch.zeros((4, 2, 24)), torch.zeros((4, 2, 4)), z, z, z, torch.zeros((2, 3)), torch.zeros(2), 8, 4)
    with pytest.raises(ValueError, match="DeviceReplayBuffer"):
        L.SACLearner(object(), None)
    critic = StackedActor(2, 22, 1)
    for kw, match in ((dict(critic=critic, critic2=critic), "critic2 is critic itself"), (dict(alpha=0.0), "alpha"), (dict(alpha=-1.0), "alpha"),
                      (dict(alpha=NAN), "alpha"), (dict(lr_alpha=-1e-3), "lr"), (dict(lr_alpha=NAN), "lr"), (dict(target_entropy=NAN), "target_entropy"),
                      (dict(target_entropy=INF), "target_entropy")):
        with pytest.raises(ValueError, match=match):                 # each fires before the buffer is looked at
            L.SACLearner(object(), None, **kw)
    four = DeviceReplayBuffer(64, 16, list(range(2)), 8, 16, 4, device="cpu")
    with pytest.raises(ValueError, match="3 action columns"):
        L.SACLearner(four, StackedActor(2, 8, 4))
    buf = DeviceReplayBuffer(64, 16, list(range(2)), 8, 16, 3, device="cpu")
    with pytest.raises(ValueError):                                  # DDPGLearner's own checks follow: a CPU ring has nothing to run on
        L.SACLearner(buf, StackedActor(2, 8, 3))


@pytest.mark.parametrize("weight", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("BnA", sorted({s[:2] for s in D.SHAPES}), ids=lambda s: "B%d-nA%d" % s)
def test_the_head_restatement_is_float64_autograd_of_l_critic(BnA, weight):
    inp = S.sac_inputs(*BnA)
    ref, t64 = S.HEAD.ref(inp, weight=weight), S.HEAD.autograd(inp, torch.float64, weight=weight)
    for k in S.HEAD.names:
        err = float(np.abs(ref[k] - t64[k]).max() / np.abs(t64[k]).max())
        assert err <= 1e-12, (k, err)
    assert ref["stats"][0] == t64["stats"][0] == inp["q1"].numel()
    for i in range(1, 8):
        assert abs(ref["stats"][i] - t64["stats"][i]) <= 1e-12 * max(abs(t64["stats"][i]), 1e-300), i
    assert all(not ref[k][..., 1:].any() for k in ("g_q1", "g_q2"))
    # alpha = 0: td3_util's head; a finished row keeps a NaN logp_next out, a running row carries it
    zero = dict(inp, log_alpha=torch.full_like(inp["log_alpha"], -float("inf")))
    two = T.HEAD.ref({k: v for k, v in inp.items() if k not in ("logp_next", "log_alpha")}, weight=weight)
    assert all(np.array_equal(S.HEAD.ref(zero, weight=weight)[k], two[k]) for k in S.HEAD.names + ("stats",))
    over = inp["done"].numpy() != 0
    bad = dict(inp, logp_next=torch.where(inp["done"] != 0, torch.tensor(NAN), inp["logp_next"]))
    assert all(np.array_equal(S.HEAD.ref(bad, weight=weight)[k], ref[k]) for k in S.HEAD.names + ("stats",))
    td = S.HEAD.ref(dict(inp, logp_next=torch.full_like(inp["logp_next"], NAN)), weight=weight)["td"]
    assert np.isnan(td[~over]).all() and np.array_equal(td[over], ref["td"][over])
    # the float32 contract, operation by operation, is a float32 evaluation of the same head
    c32 = S.contract32(inp, weight=weight)
    assert all(np.abs(c32[k] - ref[k]).max() <= 1e-5 * max(1.0, np.abs(ref[k]).max()) for k in S.HEAD.names)


@pytest.mark.parametrize("shape", ((33, 2, 8, 3, 1), (17, 1, 5, 3, 0), (9, 3, 11, 3, 1)), ids=D.shape_id)
def test_the_policy_restatements_are_float64_autograd_of_l_pi_and_l_alpha(shape):
    """The chain the learner runs -- the draw (sac_util.gauss), the seeds (ref_policy_seed), each critic's input gradient with its seed, then
    ref_policy_grad -- gives, in float64, what torch autograd gives for L_pi's gradient in the action, in log_std and L_alpha's in
    log_alpha, with real networks."""
    B, nA, Do, k, central = shape
    actor, critic = D.make_nets(nA, Do, k, central, 5)
    critic2 = D.make_nets(nA, Do, k, central, 55)[1]
    rows = D.ring_rows(B, nA, Do, k, 1)
    g = torch.Generator().manual_seed(12)
    z = torch.randn((B, nA, 4), generator=g)
    z[..., 3] = 0.0
    ls, la = -1.0 + 0.3 * torch.randn((nA, 3), generator=g), np.log(0.2) + 0.3 * torch.randn((nA,), generator=g)
    w = torch.rand((B, nA), generator=g) + 0.5
    nets = (actor, critic, critic2)
    l_c, l_pi, l_a, leaf, ex = S.losses(nets, nets[1:], ls, la, rows, w, z, z, central, torch.float64)
    ex["act_pi"].retain_grad()
    l_pi.backward(retain_graph=True)
    l_a.backward()
    # the draw
    y4 = torch.cat([leaf["actor"](rows[0].double()), torch.zeros((B, nA, 1), dtype=torch.float64)], -1).detach().numpy()
    a, logp = S.gauss(y4, ls.numpy(), z.numpy())
    assert np.abs(a - ex["act_pi"].detach().numpy()).max() <= 1e-13 and np.abs(logp - ex["logp"].detach().numpy()).max() <= 1e-12
    # the seeds in float64 and each critic's input gradient
    q1, q2 = ex["q1_pi"].detach(), ex["q2_pi"].detach()
    first = q1 < q2
    seed = -(w.double() / B)
    x = ex["x_pi"].detach().clone().requires_grad_()
    c1, c2 = leaf["critic"], leaf["critic2"]
    gx1, = torch.autograd.grad((torch.where(first, seed, torch.zeros_like(seed)) * c1(x, squash=False)[..., 0]).sum(), x)
    gx2, = torch.autograd.grad((torch.where(first, torch.zeros_like(seed), seed) * c2(x, squash=False)[..., 0]).sum(), x)
    s1, s2 = S.ref_policy_seed(q1.float().numpy(), q2.float().numpy(), w.numpy(), B)
    assert np.array_equal(s1[..., 0] != 0, first.numpy()) and np.array_equal(s2[..., 0] != 0, ~first.numpy())
    assert np.allclose(s1[..., 0] + s2[..., 0], seed.numpy(), rtol=1e-6)
    inp = dict(gx1=gx1, gx2=gx2, z=z, logp=ex["logp"].detach(), q1_pi=q1, q2_pi=q2, weight=w, log_std=ls, log_alpha=la)
    ref = S.ref_policy_grad(inp, Do, central)
    rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())          # noqa: E731
    assert rel(ref["g_a4"][..., :3], ex["act_pi"].grad.numpy()) <= 1e-11 and not ref["g_a4"][..., 3].any()
    assert rel(ref["g_log_std"], leaf["log_std"].grad.numpy()) <= 1e-11
    assert rel(ref["g_log_alpha"], leaf["log_alpha"].grad.numpy()) <= 1e-11
    # the statistics: the actor's loss is L_pi / nA, the rest plain means
    st = ref["stats"]
    assert st[0] == B * nA and abs(st[1] * nA - float(l_pi)) <= 1e-11 * abs(float(l_pi)) and abs(st[6] - float(first.double().mean())) <= 1e-15
    assert np.array_equal(S.ga32(gx1.float().numpy(), gx2.float().numpy(), Do, central)[..., :3],
                          S.own_columns(gx1.float().numpy(), Do, central) + S.own_columns(gx2.float().numpy(), Do, central))
    t32 = S.torch_policy_grad(inp, Do, central)
    assert rel(t32["g_log_std"], ref["g_log_std"]) <= 1e-4 and np.abs(t32["stats"] - st).max() <= 1e-4


@pytest.mark.parametrize("shape", S.K3[:5], ids=D.shape_id)
def test_the_draws_restatement_is_the_rollouts_expression_joined_as_ddpg_util_joins(shape):
    B, nA, Do, k, central = shape
    y4, ls, z = S.sample_arrays(shape)
    _, obs_next, act = D.batch_arrays(shape)
    for own_only in (False, True):
        x0 = D.join(obs_next, act, central).astype(np.float64)
        x, logp = S.ref_sample(y4.astype(np.float64), ls, z, x0, Do, central, own_only)
        a64, lp64 = S.torch_sample(y4, ls, z, torch.float64)
        t = lambda v: torch.from_numpy(v)                                                 # noqa: E731
        want = D.joined_pi(t(obs_next).double(), t(act).double(), t(a64), bool(central)) if own_only else D.joined(t(obs_next).double(), t(a64), bool(central))
        assert np.abs(x - want.numpy()).max() <= 1e-14 and np.abs(logp - lp64).max() <= 1e-13
    a0, _ = S.gauss(y4, np.full_like(ls, -np.inf), z)
    assert np.array_equal(a0, y4[..., :3])                                                # sigma = 0: the mean itself


@pytest.mark.parametrize("shape", S.STEP_SHAPES, ids=D.shape_id)
def test_the_whole_update_case_stays_under_the_cap_at_its_fixed_point_and_every_misreading_lies_far(shape):
    """sac_util.stepped_case's row weights are 0 where, in float64, any of these lies within KINK of 0: a pre-ReLU value of either critic
    at x_cur, of the actor at obs, of either STEPPED critic at x_pi, or |q1_pi - q2_pi|.  Under the cap, closed within MAX_ROUNDS
    (conditions on the float64 reference: the seed is the first from 0 that meets them, profiles/sac_float64.json records every seed
    tried), and each of the four misreadings lies at least 1000 yardstick mean errors from the reference.  With more than one agent so
    does each misreading of the agent index -- log_alpha, z_next (on critic 1's gradient), log_std, z_pi (on the actor's) rolled by one
    agent (measured: 1.2e4 and more) --, which is why the case's log_std rows and log_alpha values differ from agent to agent."""
    B, nA, Do, k, central = shape
    rec = json.load(open(S.PROFILE))["stepped"]
    r = rec["cases"][D.shape_id(shape)]
    c = S.stepped_case(shape)
    print(D.shape_id(shape), f"seed {c.seed}: left out {100 * c.share:.2f} % after {c.rounds} zeroing rounds")
    assert c.share < D.U.KINK_CAP and c.rounds <= O.MAX_ROUNDS and float((c.w == 0).double().mean()) == c.share
    s1, s2 = c.ref["critic"]["net"], c.ref["critic2"]["net"]
    x_cur = D.joined(c.batch[0].double(), c.batch[1].double(), central).contiguous()
    near = D.U.near_kink((s1, c.ref["x_pi"]), (s2, c.ref["x_pi"]), (c.nets[1], x_cur), (c.nets[2], x_cur), (c.nets[0], c.batch[0]))
    near |= (c.ref["pi"]["q1_pi"] - c.ref["pi"]["q2_pi"]).abs() <= D.U.KINK
    assert not (near & (c.w != 0)).any() and s1.w1.dtype == torch.float64 and not torch.equal(s1.w1, c.nets[1].w1.double())
    assert c.ref["critic"]["coef"] == c.ref["critic2"]["coef"] < 1.0 and c.ref["actor"]["coef"] < 1.0
    assert not bool(c.batch[4].all()) and not torch.equal(c.targets[0].w1, c.nets[1].w1) and not torch.equal(c.nets[1].w1, c.nets[2].w1)
    picked = float((c.ref["pi"]["q1_pi"] < c.ref["pi"]["q2_pi"]).double().mean())
    assert 0.05 < picked < 0.95 and c.stats_pi[6] == picked                             # both critics are the smaller one somewhere
    assert len({tuple(row) for row in c.log_std.tolist()}) == nA == len(set(c.log_alpha.tolist()))      # per agent, distinct
    variants = S.wrong_variants(c, central)
    assert len(variants) == 4 + (4 if nA > 1 else 0) and all((f"{k_} rolled by one agent" in variants) == (nA > 1) for k_ in S.ROLLED)
    for name, (dist, yard) in variants.items():
        ratios = {p: dist[p] / yard[p] for p in dist}
        print(D.shape_id(shape), name, "smallest ratio %.3g" % min(ratios.values()))
        assert all(yard[p] > 0.0 for p in dist) and min(ratios.values()) >= 1000.0, (name, ratios)
    assert r["seed"] == c.seed == S.STEP_SEEDS.get(shape, 0) and r["zeroing_rounds"] == c.rounds and r["shape"] == list(shape)
    assert abs(r["left_out_percent"] - 100 * c.share) <= 0.005 + 1e-9 and min(rec["sharpness"][D.shape_id(shape)].values()) >= 1000
    assert set(rec["sharpness"][D.shape_id(shape)]) == set(variants)
    tried = r["seeds_tried"]
    assert [t[0] for t in tried] == list(range(c.seed + 1)) and all(not (t[1] and t[2] < 100 * D.U.KINK_CAP) for t in tried[:-1]) and tried[-1][1]
    for seed in (0, c.seed // 2):                                                        # two of the recorded seeds, re-run
        _, share, rounds = S.try_seed(shape, seed)
        assert [round(100 * share, 2), rounds] == tried[seed][2:], seed


def test_the_profile_s_factors_are_the_rule_on_its_recorded_spread_and_the_bandit_s_n_is_the_compositions():
    rec = json.load(open(S.PROFILE))
    assert rec["factors"] == S.Y.exceptions_from(rec["head_spread"]) and set(rec["factors"]) <= {O.head_id(1, 1, True), O.head_id(1, 1, False)}
    assert set(rec["head_spread"]) == {O.head_id(B, nA, w) for B, nA in S.HEAD_SHAPES for w in (True, False)}
    for B, nA in S.HEAD_SHAPES[:-1]:
        for w in (True, False):
            got = {k: [round(float(x), 4) for x in v] for k, v in S.HEAD.spread(B, nA, w).items()}
            assert got == rec["head_spread"][O.head_id(B, nA, w)], (B, nA, w)
    assert S.HEAD.factors(161, 2, True)("g_q2") == S.Y.FACTORS
    st = rec["stepped"]
    assert set(st["cases"]) == set(st["sharpness"]) == {D.shape_id(s) for s in S.STEP_SHAPES} and set(st["kernel"]) <= set(st["cases"])
    assert S.STEP_SHAPES[:2] == S.MAIN_SHAPES and set(S.STEP_SHAPES[2:5]) < set(S.TEAM_SHAPES) and S.STEP_SHAPES[5][1:] == S.TEAM_SHAPES[2][1:]
    assert st["factors"] == S.Y.exceptions_from(st["spread"]) and set(st["spread"]) == set(st["cases"])
    for shape in S.STEP_SHAPES:
        sid = D.shape_id(shape)
        assert {k: [round(float(x), 4) for x in v] for k, v in S.stepped_spread(shape).items()} == st["spread"][sid], sid
        for name, (mean, mx) in st["kernel"].get(sid, {}).items():
            fm, fx = S.stepped_factor_of(shape)(name[6:]) if name.startswith("small.") else S.Y.FACTORS
            assert mean <= fm and mx <= fx, (shape, name)
    b = rec["bandit"]
    assert b["N"] % 10 == 0 and b["torch_closed"] >= 0.5 and {k: b[k] for k in S.BANDIT} == S.BANDIT
