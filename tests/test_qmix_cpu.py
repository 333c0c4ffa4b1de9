"""The QMIX entry points without a GPU: header, library and binding agree and the ABI version stays; bsx_qmix_members and the workspace
size; every refusal the header documents comes before any launch, in its stated order (fake addresses); the binding and QMIXLearner's
constructor refuse on the host; the numpy restatements of tests/qmix_util.py are what torch float64 autograd of the QMIX loss gives (g4
is d loss / d y4, gh is d loss / d hy) and their float32 form is a float32 evaluation of the same head; fmaf32 is a correctly rounded
fused multiply-add; the mix is monotone in every u_i and represents VDN exactly at weights written down here; the rows built to hit the
corners do hit them; the case tables of the GPU files hold on the reference alone and the whole-update cases stay under the kink cap; the
additive floor of the one-step game is 144 / 4096 and the torch composition goes below half of it; the loop's case is the issue's."""
import ctypes
import functools
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import offpolicy_util as O
import qmix_util as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bsx_qmix_members", "bsx_qmix_inputs", "bsx_qmix_head_workspace_bytes", "bsx_qmix_head")
FIELDS = ("y_cur", "y_next_online", "y_next_target", "hy_cur", "hy_next_target", "act", "rew", "done", "weight", "g4", "gh", "q", "td")
OPTIONAL = ("weight", "td")
ARG, ALIGN = -1, -2
A16, A8, A4, A1 = 4096, 4096 + 8, 4096 + 4, 4096 + 1
NAN, INF = float("nan"), float("inf")
SHAPE_IDS = dict(ids=X.shape_id)


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
    assert "#define BSX_QMIX_MAX_AGENTS 4" in hdr and L.QMIX_MAX_AGENTS == 4 == X.MAX_AGENTS and L.QMIX_EMBEDS == X.EMBEDS
    body = re.search(r"typedef struct BsxQmixIo \{(.*?)\} BsxQmixIo;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"(\w+);", body)) == FIELDS == tuple(f for f, _ in L.BsxQmixIo._fields_)
    import deep_rl_battlespace_amd as pkg
    for name in ("QMIXLearner", "QMIX_STATS", "QmixHead", "qmix_head", "qmix_head_workspace_bytes", "qmix_inputs", "qmix_members"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pkg.learner, name), name
    assert pkg.QMIX_STATS == ("n",) + X.STAT_NAMES and len(pkg.QMIX_STATS) == 8
    assert pkg.QmixHead._fields == ("g4", "gh", "q", "td", "stats")
    base = pkg.learner.ddpg._RingLearner
    assert issubclass(pkg.QMIXLearner, base) and not issubclass(pkg.QMIXLearner, pkg.DQNLearner)
    for name in ("_net", "publish", "capture", "sync", "update", "_net_state"):
        assert getattr(pkg.QMIXLearner, name) is getattr(base, name), name
    doc = pkg.QMIXLearner.__doc__
    assert "q_scale >= r_max / (1 - gamma)" in doc and "bootstrap_gamma" in doc and "decentralised" in doc
    assert "A QMIX update:" in pkg.learner.__doc__
    # DQN keeps refusing the mix by name: QMIX is a class and a head of its own
    with pytest.raises(ValueError, match="mix must be"):
        pkg.learner.dqn._mix("qmix")
    csrc = os.path.join(ROOT, "deep-rl-battlespace_amd", "csrc")
    src, shared = open(os.path.join(csrc, "bsx_qmix_head.hip")).read(), open(os.path.join(csrc, "bsx_q_head.h")).read()
    assert '#include "bsx_q_head.h"' in src and '#include "bsx_argmax4.h"' in shared and '#include "bsx_ddpg_shared.h"' in shared
    assert "__fdiv_rn" in src and "atomic" not in (src + shared).replace("no atomics", "")
    build = open(os.path.join(ROOT, "deep-rl-battlespace_amd", "build.py")).read()
    assert re.search(r'"bsx_qmix_head\.hip"\), \["-ffp-contract=off"\]', build)


def test_members_and_the_workspace():
    L = _L()
    lib, n, nb, nb0 = L.load(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    from deep_rl_battlespace_amd import learner
    for nA in range(1, 5):
        for embed in X.EMBEDS:
            assert lib.bsx_qmix_members(nA, embed, ctypes.byref(n)) == 0
            assert n.value == X.members(nA, embed) == learner.qmix_members(nA, embed) == nA * (embed // 4) + 2 * (embed // 4) + 1
    assert X.members(4, 16) == 25 and X.members(2, 8) == 9
    for bad in ((0, 8), (5, 8), (2, 0), (2, 12), (2, 32), (2, -4)):
        assert lib.bsx_qmix_members(*bad, ctypes.byref(n)) == ARG, bad
        with pytest.raises(ValueError):
            learner.qmix_members(*bad)
    assert lib.bsx_qmix_members(2, 8, None) == ARG
    # one thread per row: bsx_td_head's plan at (B, 1), whatever the team
    for B in (1, 5, 257, 300, 512, 65536, 262145, (1 << 31) - 1):
        for nA in (1, 4):
            assert lib.bsx_qmix_head_workspace_bytes(B, nA, ctypes.byref(nb)) == 0 == lib.bsx_td_head_workspace_bytes(B, 1, ctypes.byref(nb0))
            assert nb.value == nb0.value, (B, nA)
    for B_, nA_ in ((0, 2), (1 << 31, 2), (10, 0), (10, 5)):
        assert lib.bsx_qmix_head_workspace_bytes(B_, nA_, ctypes.byref(nb)) == ARG
    assert lib.bsx_qmix_head_workspace_bytes(10, 2, None) == ARG


def test_the_large_head_shapes_get_the_plans_they_are_chosen_for():
    """qmix_util.PLANS on host arithmetic alone: per shape the workspace holds one partial row of 64 bytes per workgroup and a workgroup
    takes J = ceil(tiles / workgroups) tiles of 256 batch rows; J = 2 runs at every embed and J = 3 once; one live thread in the last
    tile; the forms give every template bit both values; the widest hy is the issue's 71 MB."""
    from deep_rl_battlespace_amd import learner
    assert set(X.PLANS) == set(X.LARGE_SHAPES) and not set(X.PLANS) & set(X.HEAD_SHAPES)
    for (B, nA, embed), (tiles, J, groups) in X.PLANS.items():
        nbytes = learner.qmix_head_workspace_bytes(B, nA)
        assert nbytes % 64 == 0 and nbytes // 64 == groups, (B, nA, embed)
        assert tiles == -(-B // X.TILE) and -(-tiles // groups) == J == -(-tiles // X.MAX_BLOCKS), (B, nA, embed)
        assert B - (tiles - 1) * X.TILE == 1 and groups * J >= tiles
        print("B%d-nA%d-E%d: %d tiles, J = %d, %d workgroups, Mh = %d" % (B, nA, embed, tiles, J, groups, X.members(nA, embed)))
    assert {s[2] for s in X.LARGE_SHAPES if X.PLANS[s][1] == 2} == set(X.EMBEDS) and sorted({p[1] for p in X.PLANS.values()}) == [2, 3]
    assert all(-(-s[0] // X.TILE) <= X.MAX_BLOCKS for s in X.HEAD_SHAPES)           # what the older shapes never reach: J = 1
    assert [X.members(*s[1:]) for s in X.LARGE_SHAPES] == [4, 11, 17, 4]
    assert max(s[0] * X.members(*s[1:]) * 16 for s in X.LARGE_SHAPES) == 262145 * 17 * 16 < 72e6
    for shape in X.LARGE_SHAPES:
        forms = X.LARGE_FORMS + X.MORE_FORMS.get(shape, ())
        assert set(forms) <= set(X.FORMS) and len(set(forms)) == len(forms)
        for bit in range(3):
            assert len({bool(f[bit]) for f in forms}) == 2, (shape, bit)
    assert set(X.MORE_FORMS) == {(262145, 3, 8)} and len({f for f in X.LARGE_FORMS + X.MORE_FORMS[(262145, 3, 8)]}) == 4
    assert len(X.head_cases()) == len({X.head_case_id(c) for c in X.head_cases()}) == 4 * 8 + 4 * 2 + 2


def test_the_entries_refuse_what_the_header_documents_before_any_launch_in_its_order():
    """Fake addresses only: every call is refused before anything reaches HIP."""
    L = _L()
    lib = L.load()

    def head(B=100, nA=2, embed=8, gamma=0.95, q_scale=2.0, delta=1.0, double_q=1, ws=A16, stats=A16, io=True, **ptr):
        st = L.BsxQmixIo(**{f: ptr.get(f, None if f in OPTIONAL else A16) for f in FIELDS})
        return lib.bsx_qmix_head(ctypes.byref(st) if io else None, B, nA, embed, gamma, q_scale, delta, double_q, ws, stats, None)

    required = [f for f in FIELDS if f not in OPTIONAL + ("y_next_online",)]
    for kw in [dict(io=False), dict(ws=None), dict(stats=None)] + [{f: None} for f in required] + \
            [dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=NAN), dict(gamma=INF), dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=5), dict(nA=16)] + \
            [dict(embed=0), dict(embed=2), dict(embed=12), dict(embed=32), dict(embed=-8)] + \
            [dict(q_scale=0.0), dict(q_scale=-1.0), dict(q_scale=NAN), dict(delta=-0.5), dict(delta=NAN)] + \
            [dict(double_q=2), dict(double_q=-1), dict(y_next_online=None)]:
        assert head(**kw) == ARG, kw
    for kw in [{f: A4} for f in ("y_cur", "y_next_online", "y_next_target", "hy_cur", "hy_next_target", "act", "g4", "gh")] + \
            [{f: A8} for f in ("y_cur", "hy_cur", "act", "g4", "gh")] + [{f: A1} for f in ("rew", "weight", "q", "td")] + \
            [dict(ws=A4), dict(stats=A4), dict(y_next_online=A4, double_q=0)]:
        assert head(**kw) == ALIGN, kw
    # argument rules come before alignment rules, whichever pointer is off
    for kw in (dict(g4=A4, gamma=2.0), dict(ws=A4, B=0), dict(gh=A4, embed=5), dict(hy_cur=A4, nA=5), dict(y_cur=A4, q_scale=0.0),
               dict(act=A1, delta=-1.0), dict(rew=A1, y_next_online=None), dict(stats=A4, double_q=5)):
        assert head(**kw) == ARG, kw
    # done at any byte; y_next_online may be NULL without double Q; delta = 0 and the ends of [0, 1] are in; every team and embed
    assert head(g4=A4, done=A1, gamma=0.0, delta=0.0) == ALIGN and head(g4=A4, gamma=1.0, double_q=0, y_next_online=None, delta=INF) == ALIGN
    assert all(head(gh=A4, nA=nA, embed=e) == ALIGN for nA in range(1, 5) for e in X.EMBEDS)

    def inputs(obs=A16, obs_next=A16, B=10, nA=2, Do=8, Mh=9, x_cur=A16, x_next=A16):
        return lib.bsx_qmix_inputs(obs, obs_next, B, nA, Do, Mh, x_cur, x_next, None)
    for kw in (dict(obs=None), dict(obs_next=None), dict(x_cur=None), dict(x_next=None), dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=5),
               dict(Do=0), dict(Do=51), dict(nA=4, Do=17), dict(nA=2, Do=33), dict(Mh=0), dict(Mh=33), dict(x_cur=A1, B=0)):
        assert inputs(**kw) == ARG, kw
    for kw in (dict(obs=A1), dict(obs_next=A1), dict(x_cur=A1), dict(x_next=A1)):
        assert inputs(**kw) == ALIGN, kw


def test_the_binding_and_the_learners_constructor_refuse_on_the_host():
    from deep_rl_battlespace_amd import learner as L
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    from deep_rl_battlespace_amd.rollout import StackedActor
    r4, h4, r2, flag = torch.zeros((4, 2, 4)), torch.zeros((4, 9, 4)), torch.zeros((4, 2)), torch.zeros((4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        L.qmix_head(r4, r4, h4, h4, r4, r2, flag, 0.9, embed=8, q_scale=2.0)
    with pytest.raises(ValueError, match="GPU"):
        L.qmix_inputs(torch.zeros((4, 2, 8)), torch.zeros((4, 2, 8)), 9)
    with pytest.raises(ValueError, match=r"y_cur must be a float32 \[B, nA, 4\] tensor"):
        L.qmix_head(r2, r4, h4, h4, r4, r2, flag, 0.9, embed=8, q_scale=2.0)
    for kw, match in ((dict(embed=8, q_scale=0.0), "q_scale"), (dict(embed=8, q_scale=NAN), "q_scale"), (dict(embed=8, q_scale=2.0, huber_delta=-1.0), "huber_delta"),
                      (dict(embed=6, q_scale=2.0), "embed must be"), (dict(embed=32, q_scale=2.0), "embed must be")):
        with pytest.raises(ValueError, match=match):
            L.qmix_head(r4, r4, h4, h4, r4, r2, flag, 0.9, **kw)
    with pytest.raises(ValueError, match="1 .. 4 agents"):
        L.qmix_head(torch.zeros((4, 5, 4)), r4, h4, h4, r4, r2, flag, 0.9, embed=8, q_scale=2.0)
    with pytest.raises(ValueError, match="DeviceReplayBuffer"):
        L.QMIXLearner(object(), None, q_scale=2.0)
    with pytest.raises(TypeError):                                   # q_scale has no default: the bound of Q is the caller's choice
        L.QMIXLearner(object(), None)
    ring = lambda nA, Do, k=4: DeviceReplayBuffer(64, 16, list(range(nA)), Do, Do * nA, k, device="cpu")     # noqa: E731
    four, net = ring(2, 8), StackedActor(2, 8, 4)
    with pytest.raises(ValueError, match="n_actions == 4"):
        L.QMIXLearner(ring(2, 8, 3), StackedActor(2, 8, 3), q_scale=2.0)
    for embed in (0, 2, 6, 12, 32):
        with pytest.raises(ValueError, match="embed must be"):
            L.QMIXLearner(four, net, embed=embed, q_scale=2.0)
    with pytest.raises(ValueError, match="1 .. 4 agents"):
        L.QMIXLearner(ring(5, 8), StackedActor(5, 8, 4), q_scale=2.0)
    with pytest.raises(ValueError, match="joint observation"):      # S = 4 x 17 = 68 > 64
        L.QMIXLearner(ring(4, 17), StackedActor(4, 17, 4), q_scale=2.0)
    for bad in (StackedActor(2, 8, 3), StackedActor(2, 9, 4), StackedActor(3, 8, 4), object()):
        with pytest.raises(ValueError, match="qnet must be a StackedActor"):
            L.QMIXLearner(four, bad, q_scale=2.0)
    for bad in (StackedActor(8, 16, 4), StackedActor(9, 15, 4), StackedActor(9, 16, 3), StackedActor(5, 16, 4), object()):
        with pytest.raises(ValueError, match="mixer must be a StackedActor"):
            L.QMIXLearner(four, net, bad, q_scale=2.0)
    with pytest.raises(ValueError, match="mixer must be a StackedActor"):      # a mixer of embed 8 at embed 4
        L.QMIXLearner(four, net, StackedActor(9, 16, 4), embed=4, q_scale=2.0)
    for kw, match in ((dict(q_scale=0.0), "q_scale"), (dict(q_scale=-3.0), "q_scale"), (dict(q_scale=2.0, huber_delta=-1.0), "huber_delta"),
                      (dict(q_scale=2.0, gamma=1.5), "gamma"), (dict(q_scale=2.0, updates=0), "updates")):
        with pytest.raises(ValueError, match=match):
            L.QMIXLearner(four, net, **kw)
    with pytest.raises(ValueError):                                  # the fused MLP's own checks follow: a CPU ring has nothing to run on
        L.QMIXLearner(four, net, StackedActor(9, 16, 4), q_scale=2.0)


def test_fmaf32_is_a_correctly_rounded_fused_multiply_add():
    """Against exact rational arithmetic on random operands, on sums that cancel, and on a case built so that rounding the float64 sum
    first would round twice: a = 1 + 2^-12, x = 1 + 2^-12 (p = 1 + 2^-11 + 2^-24, exact), y = 2^-60: the exact sum lies just ABOVE the
    midpoint of two float32, float64 rounds it ONTO the midpoint, and ties-to-even would then round down."""
    g = np.random.default_rng(5)
    a, x, y = (g.standard_normal(4000).astype(np.float32) for _ in range(3))
    y[:1000] = (-(a[:1000].astype(np.float64) * x[:1000])).astype(np.float32)       # cancelling sums
    a = np.concatenate([a, np.float32([1 + 2.0 ** -12, 1 + 2.0 ** -12])])
    x = np.concatenate([x, np.float32([1 + 2.0 ** -12, 1 + 2.0 ** -12])])
    y = np.concatenate([y, np.float32([2.0 ** -60, -2.0 ** -60])])
    got = X.fmaf32(a, x, y)

    def exact(i):
        v = Fraction(float(a[i])) * Fraction(float(x[i])) + Fraction(float(y[i]))
        lo = np.float32(float(v))                                                   # float(v) rounds the rational ONCE to float64: refine below
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - v), int(c.view(np.int32)) & 1))
        return best
    want = np.array([exact(i) for i in range(len(a))], np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    naive = (a.astype(np.float64) * x + y).astype(np.float32)
    assert naive[-2] != got[-2] and got[-2] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)       # the double rounding is real, and avoided
    assert np.isnan(X.fmaf32(np.float32([NAN]), np.float32([1]), np.float32([1])))[0] and X.fmaf32(np.float32([INF]), np.float32([1]), np.float32([1]))[0] == INF


@pytest.mark.parametrize("form", X.FORMS, ids=X.form_id)
@pytest.mark.parametrize("shape", X.HEAD_SHAPES, **SHAPE_IDS)
def test_the_restatement_is_float64_autograd_of_the_qmix_loss(shape, form):
    """ref64 against torch float64 autograd from the two networks' tanh rows: g4 equals d loss / d y4 and gh d loss / d hy (no hypernet
    value of the inputs is 0), q and td the composition's, the statistics its means; contract32, operation by operation in float32, is a
    float32 evaluation of the same head."""
    B, nA, embed = shape
    kw = X._kw(form)
    inp = X.head_inputs(B, nA, embed)
    assert float(inp["hy_cur"].abs().min()) > 0
    ref, t64, c32 = X.ref64(inp, embed, **kw), X.torch_head(inp, torch.float64, embed, **kw), X.contract32(inp, embed, **kw)
    for k in X.OUTS:
        err = float(np.abs(ref[k] - t64[k]).max() / np.abs(t64[k]).max())
        assert err <= 1e-12, (k, err)
        assert c32[k].dtype == np.float32 and c32[k].shape == ref[k].shape
        assert np.abs(c32[k] - ref[k]).max() <= 2e-5 * max(1.0, np.abs(ref[k]).max()), k
    assert ref["stats"][0] == t64["stats"][0] == B
    for i in range(1, 8):
        assert abs(ref["stats"][i] - t64["stats"][i]) <= 1e-12 * max(abs(t64["stats"][i]), 1e-300), i
    assert ((ref["g4"] != 0).sum(-1) <= 1).all() and (ref["gh"][:, -1, 1:] == 0).all()
    assert all((ref[k] == ref[k][:, :1]).all() for k in ("q", "td"))
    if B > 100:
        over = (inp["done"] != 0).all(1)
        assert 0.2 < float(over.double().mean()) < 0.5 and (nA == 1 or bool(((inp["done"] != 0).any(1) & ~over).any()))
        if form[1]:
            inside = np.abs(ref["q"] - ref["td"]) <= form[1]
            assert inside.any() and not inside.all()                  # both sides of the Huber corner


def test_the_mix_is_monotone_in_every_plane_and_is_vdn_at_written_down_weights():
    """Monotone: raising any u_i never lowers tot, in float64 and in the float32 contract, on random hypernet rows of every team and
    embed.  VDN: with W1[i][e] = 1 at e = i and 0 elsewhere, b1 = 1 (every pre_e = u_i + 1 >= 0 stays on the identity branch), w2 = 1 on
    the first nA units and 0 beyond, b2 = -nA, tot is EXACTLY u_0 + .. + u_{nA-1}: the additive mix is inside the family."""
    g = np.random.default_rng(11)
    for nA in range(1, 5):
        for embed in X.EMBEDS:
            Mh, Bn = X.members(nA, embed), 200
            hy = np.tanh(g.standard_normal((Bn, Mh, 4)))
            u = np.tanh(g.standard_normal((Bn, nA)))
            base64, base32 = X.mix64(u, hy, embed)[0], X.mix32(u.astype(np.float32), hy.astype(np.float32), embed)[0]
            for i in range(nA):
                up = u.copy()
                up[:, i] += np.abs(g.standard_normal(Bn)) * 0.3
                assert (X.mix64(up, hy, embed)[0] >= base64).all(), (nA, embed, i)
                assert (X.mix32(up.astype(np.float32), hy.astype(np.float32), embed)[0] >= base32 - 1e-6).all(), (nA, embed, i)
            if embed >= nA:
                m = embed // 4
                t1 = np.zeros((Bn, nA, embed), np.float32)
                for i in range(nA):
                    t1[:, i, i] = -1.0                                              # |.| makes it 1
                b1 = np.ones((Bn, embed), np.float32)
                t2 = np.zeros((Bn, embed), np.float32)
                t2[:, :nA] = 1.0
                last = np.zeros((Bn, 1, 4), np.float32)
                last[:, 0, 0] = -nA
                vdn = np.concatenate([t1.reshape(Bn, nA * m, 4), b1.reshape(Bn, m, 4), t2.reshape(Bn, m, 4), last], 1)
                u32 = (np.round(u * 4096) / 4096).astype(np.float32)                 # 13-bit fractions: their float32 sums are exact
                want = u32.astype(np.float64).sum(1)
                assert np.array_equal(X.mix32(u32, vdn, embed)[0].astype(np.float64), want) and np.array_equal(X.mix64(u32.astype(np.float64), vdn.astype(np.float64), embed)[0], want)
    # the negative branch: ELU's shape -- slope 1 at 0, floor -1, C1 -- and a NaN stays a NaN
    x = np.float32([-1e6, -1.0, -1e-3, -0.0, 0.0, 1e-3, 2.0, NAN])
    hy = np.zeros((len(x), X.members(1, 4), 4), np.float32)
    hy[:, 1, 0] = x                                                                 # b1_0 = x, every W1 0
    hy[:, 2, 0] = 1.0                                                               # w2_0 = 1
    tot, h, sl = X.mix32(np.zeros((len(x), 1), np.float32), hy, 4)
    assert np.array_equal(h[:-1, 0], np.float32([x[0] * (np.float32(1) / (np.float32(1) - x[0])), -0.5, x[2] * (np.float32(1) / (np.float32(1) - x[2])), -0.0, 0.0, 1e-3, 2.0]))
    assert h[0, 0] > -1.0 - 1e-6 and np.array_equal(sl[3:7, 0], np.float32([1, 1, 1, 1])) and sl[1, 0] == 0.25 and np.isnan(h[-1, 0]) and np.isnan(tot[-1])


GAMMA32 = float(np.float32(X.GAMMA))


@pytest.mark.parametrize("shape", X.HEAD_SHAPES, **SHAPE_IDS)
def test_the_corner_rows_hit_the_corners_they_are_built_for(shape):
    B, nA, embed = shape
    inp, fitted = X.corner_inputs(B, nA, embed)
    assert fitted == tuple(c for r, c in enumerate(X.CORNERS) if r < B and not (r in X.NEEDS_TEAM and nA == 1)) and len(fitted) >= 1
    if B < len(X.CORNERS):
        return
    m = embed // 4
    k = nA * m
    for delta in (0.0, X.DELTA):
        c = X.contract32(inp, embed, delta=delta)
        d = c["q"] - c["td"]
        col = lambda b, i=0: int(np.flatnonzero(c["g4"][b, i] != 0)[0])             # noqa: E731
        assert col(0) == 1 and col(1) == 2                                          # the first maximum; a NaN is the maximum
        R2 = functools.reduce(lambda s_, r_: np.float32(s_ + r_), inp["rew"][2].numpy())
        assert np.isfinite(c["td"][2]).all() and (c["td"][2] == R2).all()           # a finished team: y is the summed reward, NaN and inf stay out
        assert np.isfinite(c["td"][3]).all() and inp["done"][3, 0] == 1 and not bool(inp["done"][3, 1:].any())
        assert (d[4] == 1.0).all() and (d[5] == -1.0).all()                         # |d| exactly delta
        if delta:                                                                   # the corner itself is not clipped: the slope of d^2
            assert c["gh"][4, k + 2 * m, 0] == np.float32(2.0 / B) * np.float32(X.Q_SCALE) == -c["gh"][5, k + 2 * m, 0]
        u6 = X.Q._take(inp["y_cur"].numpy(), X.argmax4(inp["act"].numpy()))[6:7]
        tot, h, sl = X.mix32(u6, inp["hy_cur"].numpy()[6:7], embed)
        assert not h.any() and (sl == 1).all() and not np.signbit(h).any()          # pre exactly 0: the second branch, h = +0, slope 1
        tot, h, sl = X.mix32(X.Q._take(inp["y_cur"].numpy(), X.argmax4(inp["act"].numpy()))[7:8], inp["hy_cur"].numpy()[7:8], embed)
        assert (h < -0.998).all() and (h > -1).all() and (sl < 2e-6).all() and (sl > 1e-8).all()      # far below 0, and no denormal
        g8 = c["gh"][8]
        assert not g8[:k, 0].any() and not g8[:k, 1].any() and g8[:k, 2].all() and not g8[:k, 3].any()      # sgn(+-0) = 0: no gradient through |0|
        assert not g8[k + m:k + 2 * m, 0].any() and not g8[k + m:k + 2 * m, 3].any() and g8[k + m:k + 2 * m, 1:3].all() and g8[k:k + m, 1:3].all()
        assert np.isnan(c["g4"][9]).sum() == nA and np.isnan(c["gh"][9, :, 0]).all() and not np.isnan(c["td"][9]).any() and np.isnan(d[9]).all()
        assert not c["gh"][9, k + 2 * m, 1:].view(np.int32).any()                   # +0 beside a NaN
        assert all(X.same_bits_or_nan(c[key], np.repeat(c[key][:, :1], nA, 1)) for key in ("q", "td"))
    # double Q picks by the online rows -- ties and NaN by argmax4's rule -- and values by the target rows
    f = {key: v.numpy() for key, v in inp.items()}
    an = X.argmax4(f["y_next_online"])
    assert (an[10] == 0).all() and (an[11] == 1).all()
    un = X.Q._take(f["y_next_target"], an)
    assert (un[10] == -0.5).all() and (un[11] == 0.25).all()
    for b in (10, 11):
        tot_n = X.mix32(un[b:b + 1], f["hy_next_target"][b:b + 1], embed)[0]
        want = X.fmaf32(np.float32([GAMMA32]), (np.float32(X.Q_SCALE) * tot_n).astype(np.float32), np.float32([f["rew"][b].astype(np.float64).sum()]))
        if nA == 1:
            assert X.contract32(inp, embed)["td"][b, 0] == want[0]
    single = X.contract32(inp, embed, double=False)["td"]
    assert not np.array_equal(single[10], X.contract32(inp, embed)["td"][10])


def test_the_case_tables_hold_on_the_reference_alone_and_the_whole_update_cases_stay_under_the_kink_cap():
    """The GPU files' tables; and per team the float64 reference ALONE leaves out at most a quarter of the rows at the case's seed --
    the first from 0 that qualifies --, closes within offpolicy_util.MAX_ROUNDS, and no arg-max margin lies below KINK."""
    assert X.HEAD_SHAPES == ((1, 1, 4), (5, 3, 8), (257, 2, 8), (300, 4, 16)) and len(X.FORMS) == 8 and len(set(X.FORMS)) == 8 and len(X.CORNERS) == 12
    assert X.TEAMS == ((1, 5, 4), (2, 8, 8), (3, 11, 4), (4, 14, 16)) and X.FLOAT64_TEAMS == ((1, 5, 4), (2, 8, 8), (3, 11, 4)) and X.B == 64
    assert X.KINK == 1e-4 and X.KINK_CAP == 0.25
    rec = json.load(open(X.PROFILE))
    for team in X.FLOAT64_TEAMS:
        seed = X.STEP_SEEDS.get(team, 0)
        for s in range(seed):
            assert X.try_seed(team, s)[0] is None, (team, s)
        c = X.stepped_case(team)
        print(X.team_id(team), f"seed {c.seed}: left out {100 * c.share:.2f} % of the rows after {c.rounds} rounds; smallest margin {c.margin:.2e}")
        assert c.share <= X.KINK_CAP and c.rounds <= O.MAX_ROUNDS and c.margin >= X.KINK
        assert not (X.near_kink(c.nets, c.batch, c.ref, c.embed) & (c.w != 0)).any()
        assert float((c.w != 0).double().mean()) >= 0.75 and not torch.equal(c.nets[2].w1, c.qnet.w1) and not torch.equal(c.nets[3].w1, c.mixer.w1)
        assert c.ref["net"]["coef"] < 1.0 and c.ref["mix"]["coef"] < 1.0             # both clips are active
        assert not bool(c.batch[4].all()) and bool(c.batch[4].any())
        r = rec["stepped"]["cases"][X.team_id(team)]
        assert r["seed"] == c.seed and abs(r["left_out_percent"] - 100 * c.share) <= 0.005 + 1e-9 and r["zeroing_rounds"] == c.rounds
        for name, (mean, mx) in rec["stepped"]["kernel"].get(X.team_id(team), {}).items():
            assert mean <= X.Y.FACTORS[0] and mx <= X.Y.FACTORS[1], (team, name)
    assert "factors" not in rec or rec["factors"] == {}                           # nothing is held to a wider factor than (2, 4)


def test_the_additive_floor_is_derived_and_the_torch_composition_goes_below_half_of_it():
    """The floor by least squares over all additive tables q1(a) + q2(b): 144 / 4096.  The learning check's conditions on the float32
    composition alone, at the recorded update count, for both embeds: the exact table error of Q_tot over the 16 cells is below half the
    floor and the greedy joint action is (0, 0); the profile's records of the other embed, of float64 and of the learner say the same."""
    b = X.TASK
    A = np.zeros((16, 8))
    for a in range(4):
        for c in range(4):
            A[4 * a + c, a] = A[4 * a + c, 4 + c] = 1.0
    t = X.task_table().reshape(-1)
    fit = A @ np.linalg.lstsq(A, t, rcond=None)[0]
    assert abs(((fit - t) ** 2).mean() - X.VDN_FLOOR) <= 1e-12 and X.VDN_FLOOR == 144.0 / 4096.0
    rows = X.task_rows()
    assert bool(rows[4].all()) and bool((rows[0] == rows[0][0]).all()) and abs(float((rows[2][:, 0] > 0).float().mean()) - 1 / 16) < 0.02
    assert b["N"] == 600 and b["rows"] == 2048 and b["B"] == 256 and b["q_scale"] == 2.0 and b["lr"] == 2e-3 and 1.0 <= b["q_scale"]
    embed = b["embeds"][0]
    start = X.table_error(X.net_table(*X.task_nets(embed), embed))
    q, mx, losses = X.task_twin(embed, X.task_draws(b["N"]), torch.float32)
    table = X.net_table(q, mx, embed)
    err = X.table_error(table)
    print(f"embed {embed} float32: batch loss {losses[0]:.4f} -> {losses[-1]:.4f}; table error {start:.4f} -> {err:.5f} (floor {X.VDN_FLOOR:.4f})")
    assert err < 0.5 * X.VDN_FLOOR < start and np.unravel_index(table.argmax(), (4, 4)) == (0, 0)
    with torch.no_grad():
        assert q(X.task_obs()[None])[0].argmax(-1).tolist() == [0, 0]               # each plane's own arg-max: decentralised play
    # the other embed and float64 are the profile's (tools/measure_qmix.py --float64 runs them): every recorded twin is under half the floor
    rec = json.load(open(X.PROFILE))["task"]
    assert rec["additive_floor"] == X.VDN_FLOOR and set(rec["twin"]) == {"embed%d" % e for e in b["embeds"]}
    assert abs(rec["twin"]["embed%d" % embed]["float32"]["table_error"] - err) <= 1e-3
    for per in rec["twin"].values():
        for name in ("float32", "float64"):
            assert per[name]["table_error"] < 0.5 * X.VDN_FLOOR < per["initial_table_error"] and per[name]["greedy_joint_action"] == [0, 0]
    for fig in rec["learner"].values():
        assert fig["table_error"] < 0.5 * X.VDN_FLOOR and abs(fig["table_error"] - fig["float64_twin_table_error"]) <= fig["bound"]


def test_the_loops_case_is_the_issues():
    c = X.LOOP
    assert (c["n"], c["E"], c["T"], c["nstep"], c["iters"], c["noise_std"], c["M"]) == (2, 64, 8, 3, 3, 0.3, 4096)
    assert c["E"] * c["T"] >= c["B"] and c["embed"] in X.EMBEDS and c["updates"] >= 1
