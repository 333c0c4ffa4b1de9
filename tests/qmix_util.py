"""What the tests of the QMIX head (csrc/bsx_qmix_head.hip: learner.qmix_head) and of QMIXLearner share, on top of tests/dqn_util.py,
offpolicy_util.py and yardstick_util.py:

  members, split, fmaf32, mix32, contract32   the header's contract of bsx_qmix_head restated in numpy float32, operation by operation:
                     g4, gh, q and td are held to it BIT FOR BIT (every operation is specified).  fmaf32 is a correctly rounded float32
                     fused multiply-add: the product is exact in float64, the sum is rounded to odd there (TwoSum gives the error's
                     sign), so the second rounding to float32 is the single rounding of the exact result
  mix64, ref64       the same contract in float64, statistics included
  torch_mix, torch_loss, torch_head   the mix and the QMIX loss as a torch user writes them; autograd from the two networks' tanh rows:
                     in float64 the check of the restatement (g4 = d loss / d y4, gh = d loss / d hy), in float32 the statistics' yardstick
  head_inputs, corner_inputs, HEAD_SHAPES, FORMS   the head suite's inputs, the rows built to hit the contract's corners, its case table
  LARGE_SHAPES, PLANS, LARGE_FORMS, MORE_FORMS, head_cases   the shapes at which a workgroup takes J = 2 or 3 tiles, with the plan each must get
  guarded_head, guarded_inputs   learner.qmix_head / qmix_inputs with every array between guard slabs
  TEAMS, FLOAT64_TEAMS, learner_case, update_reference, near_kink, try_seed, stepped_case   a whole update on the CPU in float64 (the
                     reference) and float32 (the yardstick): autograd through both StackedActors, offpolicy_util.first_step per network
  Hand, snapshot, learner_and_hand   one update by hand from the public primitives, under a QMIXLearner's names
  the pay-off VDN cannot fit   TASK, task_rows, task_nets, task_twin, table_error: a one-step game whose team pay-off is 1 only when both
                     planes play action 0
  LOOP               the documented loop's case

Nothing here imports the native library at import time."""
import copy
import functools
import os
import types

import numpy as np
import torch

import actor_grad_util as U
import ddpg_util as D
import dqn_util as Q
import mlp_grad_util as M
import offpolicy_util as O
import qlearn_util as QL
import yardstick_util as Y

PARAMS = U.PARAMS
GAMMA = O.GAMMA
Q_SCALE = 4.0                       # a power of two: q_scale * tot is exact, which lets a row sit EXACTLY on a Huber corner
DELTA = 1.0
NAN, INF = float("nan"), float("inf")
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "qmix_float64.json")
STAT_NAMES = ("loss", "q_tot", "target", "abs_td", "done", "weight", "greedy")      # stats[1..7], learner.QMIX_STATS[1:]
EMBEDS = (4, 8, 16)
MAX_AGENTS = 4
# (B, nA, embed): one row of one plane; an odd team; one row past a 256-row tile; the widest team and mix, two workgroups
HEAD_SHAPES = ((1, 1, 4), (5, 3, 8), (257, 2, 8), (300, 4, 16))
# (double, huber delta, weighted)
FORMS = tuple((dbl, delta, w) for dbl in (True, False) for delta in (0.0, DELTA) for w in (True, False))
# The smallest shapes at which a workgroup takes J > 1 tiles (bsx_ddpg_shared.h: plan_of(B, 1), one thread per batch row: tiles of TILE
# rows, at most MAX_BLOCKS workgroups), (B, nA, embed) -> (tiles, J, workgroups): J = 2 at every embed -- one live thread in the last
# workgroup and one tile past `tiles` --, and J = 3, which tells blockIdx * J from a hard-coded 2.  The widest rows are (262145, 2, 16)'s:
# Mh = 17 members, an hy of 71 MB.  LARGE_FORMS run at every large shape, MORE_FORMS as well at (262145, 3, 8): every template bit takes
# both values
TILE, MAX_BLOCKS = Q.TILE, Q.MAX_BLOCKS
LARGE_SHAPES = ((262145, 1, 4), (262145, 3, 8), (262145, 2, 16), (524289, 1, 4))
PLANS = {(262145, 1, 4): (1025, 2, 513), (262145, 3, 8): (1025, 2, 513), (262145, 2, 16): (1025, 2, 513), (524289, 1, 4): (2049, 3, 683)}
LARGE_FORMS = ((True, DELTA, True), (False, 0.0, False))
MORE_FORMS = {(262145, 3, 8): ((True, 0.0, False), (False, DELTA, True))}
LARGE_PERMS = Q.LARGE_PERMS         # the yardstick's row orders beside the given one at the LARGE_SHAPES (8 elsewhere)
OUTS = ("g4", "gh", "q", "td")
argmax4, same_bits_or_nan = Q.argmax4, Q.same_bits_or_nan


def shape_id(s):
    return "B%d-nA%d-E%d" % s


def form_id(form):
    dbl, delta, w = form
    return "%s-%s-%s" % ("double" if dbl else "single", "huber" if delta else "mse", "weighted" if w else "plain")


def head_cases():
    """[(shape, form)] of the head suite: every form at HEAD_SHAPES, LARGE_FORMS and MORE_FORMS at LARGE_SHAPES."""
    return [(s, f) for s in HEAD_SHAPES for f in FORMS] + [(s, f) for s in LARGE_SHAPES for f in LARGE_FORMS + MORE_FORMS.get(s, ())]


def head_case_id(c):
    return shape_id(c[0]) + "-" + form_id(c[1])


def members(nA, embed):
    m = embed // 4
    return nA * m + 2 * m + 1


# ------------------------------------------------------------------------------------------------ the head's contract
def fmaf32(a, x, y):
    """fmaf(a, x, y) of float32 arrays, correctly rounded: p = a x is exact in float64; s = RN64(p + y) with TwoSum's error e; where e is
    not 0 and s's last bit is even, s moves one float64 step towards e (round to odd); float32(s) is then the exact sum rounded once."""
    a, x, y = (np.asarray(v, np.float32).astype(np.float64) for v in (a, x, y))
    with np.errstate(all="ignore"):
        p = a * x
        s = p + y
        bb = s - p
        e = (p - (s - bb)) + (y - bb)
        even = (s.view(np.int64) & 1) == 0
        move = np.isfinite(s) & np.isfinite(e) & (e != 0) & even
        s = np.where(move, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def split(hy, nA, embed):
    """hy [B, Mh, 4] -> (t1 [B, nA, E], b1 [B, E], t2 [B, E], b2 [B]): the raw hypernet values at W1's, b1's, w2's and b2's places."""
    B, m = hy.shape[0], embed // 4
    k = nA * m
    return hy[:, :k].reshape(B, nA, embed), hy[:, k:k + m].reshape(B, embed), hy[:, k + m:k + 2 * m].reshape(B, embed), hy[:, k + 2 * m, 0]


def mix32(u, hy, embed):
    """The header's mix(u, hy), steps 1 to 3, in float32 -> (tot [B], h [B, E], slope [B, E])."""
    f32 = np.float32
    nA = u.shape[1]
    t1, b1, t2, b2 = split(hy, nA, embed)
    W1, w2 = np.abs(t1), np.abs(t2)
    with np.errstate(all="ignore"):
        pre = b1.astype(f32).copy()
        for i in range(nA):
            pre = fmaf32(u[:, i, None], W1[:, i], pre)
        up = pre > 0
        r = (f32(1.0) / (f32(1.0) - pre).astype(f32)).astype(f32)
        h = np.where(up, pre, (pre * r).astype(f32)).astype(f32)
        sl = np.where(up, f32(1.0), (r * r).astype(f32)).astype(f32)
        tot = b2.astype(f32).copy()
        for e in range(embed):
            tot = fmaf32(h[:, e], w2[:, e], tot)
    return tot, h, sl


def _sgn(t):
    return (t > 0).astype(np.float32) - (t < 0).astype(np.float32)


def contract32(inp, embed, gamma=GAMMA, q_scale=Q_SCALE, delta=0.0, double=True, weight=True):
    """include/battlespace_hip.h's bsx_qmix_head per batch row, in numpy float32, every operation rounded once -> dict(g4, gh, q, td)."""
    f = {k: v.numpy() for k, v in inp.items()}
    f32 = np.float32
    B, nA = f["rew"].shape
    m = embed // 4
    qs = f32(q_scale)
    with np.errstate(all="ignore"):
        a = argmax4(f["act"])
        an = argmax4(f["y_next_online"] if double else f["y_next_target"])
        fin = f["done"] != 0
        un = np.where(fin, f32(0.0), Q._take(f["y_next_target"], an)).astype(f32)
        tot_n, _, _ = mix32(un, f["hy_next_target"], embed)
        N = np.where(fin.all(1), f32(0.0), (qs * tot_n).astype(f32)).astype(f32)
        R = f["rew"][:, 0].astype(f32).copy()
        for i in range(1, nA):
            R = (R + f["rew"][:, i]).astype(f32)
        u = Q._take(f["y_cur"], a).astype(f32)
        tot, h, sl = mix32(u, f["hy_cur"], embed)
        Qt = (qs * tot).astype(f32)
        w = f["weight"][:, 0].astype(f32) if weight else np.ones(B, f32)
        y, G = QL.tail32(fmaf32, Qt, N, R, w, gamma, q_scale, delta, B)
        t1, _, t2, _ = split(f["hy_cur"], nA, embed)
        W1 = np.abs(t1)
        ws = (np.abs(t2) * sl).astype(f32)
        gh = np.zeros((B, members(nA, embed), 4), f32)
        g4 = np.zeros((B, nA, 4), f32)
        k = nA * m
        for i in range(nA):
            S = np.zeros(B, f32)
            for e in range(embed):
                S = fmaf32(ws[:, e], W1[:, i, e], S)
            np.put_along_axis(g4[:, i], a[:, i, None], (G * S).astype(f32)[:, None], -1)
            gw1 = ((G[:, None] * (ws * u[:, i, None]).astype(f32)).astype(f32) * _sgn(t1[:, i])).astype(f32)
            gh[:, i * m:(i + 1) * m] = gw1.reshape(B, m, 4)
        gh[:, k:k + m] = (G[:, None] * ws).astype(f32).reshape(B, m, 4)
        gh[:, k + m:k + 2 * m] = ((G[:, None] * h).astype(f32) * _sgn(t2)).astype(f32).reshape(B, m, 4)
        gh[:, k + 2 * m, 0] = G
    rep = lambda x: np.repeat(x[:, None], nA, 1).astype(f32)                        # noqa: E731
    return dict(g4=g4, gh=gh, q=rep(Qt), td=rep(y))


def mix64(u, hy, embed):
    """mix(u, hy) in float64 -> (tot [B], h, slope [B, E])."""
    t1, b1, t2, b2 = split(hy, u.shape[1], embed)
    with np.errstate(all="ignore"):
        pre = b1 + (u[:, :, None] * np.abs(t1)).sum(1)
        r = 1.0 / (1.0 - np.minimum(pre, 0.0))
        h = np.where(pre > 0, pre, pre * r)
        sl = np.where(pre > 0, 1.0, r * r)
        return b2 + (h * np.abs(t2)).sum(1), h, sl


def ref64(inp, embed, gamma=GAMMA, q_scale=Q_SCALE, delta=0.0, double=True, weight=True):
    """The same contract in float64 numpy on the inputs as given -> dict(g4, gh, q, td, stats [8])."""
    f = {k: (v.double().numpy() if v.is_floating_point() else v.numpy()) for k, v in inp.items()}
    B, nA = f["rew"].shape
    m = embed // 4
    gamma = float(np.float32(gamma))
    with np.errstate(all="ignore"):
        a = argmax4(f["act"])
        an = argmax4(f["y_next_online"] if double else f["y_next_target"])
        fin = f["done"] != 0
        over = fin.all(1)
        un = np.where(fin, 0.0, Q._take(f["y_next_target"], an))
        N = np.where(over, 0.0, q_scale * mix64(un, f["hy_next_target"], embed)[0])
        u = Q._take(f["y_cur"], a)
        tot, h, sl = mix64(u, f["hy_cur"], embed)
        Qt = q_scale * tot
        w = f["weight"][:, 0] if weight else np.ones(B)
        y, d, loss, G = QL.tail64(Qt, N, f["rew"].sum(1), w, gamma, q_scale, delta, B)
        t1, _, t2, _ = split(f["hy_cur"], nA, embed)
        ws = np.abs(t2) * sl
        g4 = np.zeros((B, nA, 4))
        np.put_along_axis(g4, a[..., None], (G[:, None] * (ws[:, None, :] * np.abs(t1)).sum(-1))[..., None], -1)
        gh = np.zeros((B, members(nA, embed), 4))
        k = nA * m
        gh[:, :k] = (G[:, None, None] * ws[:, None, :] * u[:, :, None] * np.sign(t1)).reshape(B, k, 4)
        gh[:, k:k + m] = (G[:, None] * ws).reshape(B, m, 4)
        gh[:, k + m:k + 2 * m] = (G[:, None] * h * np.sign(t2)).reshape(B, m, 4)
        gh[:, k + 2 * m, 0] = G
        stats = QL.stats64(float(B), w, loss, Qt, y, d, over, (a == argmax4(f["y_cur"])).mean(1))
    rep = lambda x: np.repeat(x[:, None], nA, 1)                                    # noqa: E731
    return dict(g4=g4, gh=gh, q=rep(Qt), td=rep(y), stats=stats)


def torch_mix(u, hy, embed):
    """Q_tot / q_scale as a torch user writes the mix: u [B, nA], hy [B, Mh, 4] -> [B].  x / (1 - x) below 0, evaluated on min(x, 0) so
    that the branch not taken has a finite derivative."""
    B, nA = u.shape
    m = embed // 4
    k = nA * m
    W1, b1 = hy[:, :k].reshape(B, nA, embed).abs(), hy[:, k:k + m].reshape(B, embed)
    w2, b2 = hy[:, k + m:k + 2 * m].reshape(B, embed).abs(), hy[:, k + 2 * m, 0]
    pre = b1 + (u[:, :, None] * W1).sum(1)
    neg = pre.clamp(max=0.0)
    h = torch.where(pre > 0, pre, neg / (1.0 - neg))
    return b2 + (h * w2).sum(1)


def torch_loss(y_cur, hy_cur, y_on, y_tg, hy_tg, act, rew, done, w, dtype, gamma, q_scale, delta, double, embed):
    """The QMIX loss from the five tanh row tensors -> (loss = mean_b w l(Q_tot - y), Q_tot [B], y [B], per-row w l(d), w [B])."""
    a = act.argmax(-1, keepdim=True)
    Qt = q_scale * torch_mix(y_cur.gather(-1, a)[..., 0], hy_cur, embed)
    with torch.no_grad():
        nxt = y_tg.gather(-1, (y_on if double else y_tg).argmax(-1, keepdim=True))[..., 0]
        un = torch.where(done != 0, torch.zeros((), dtype=dtype), nxt)
        N = torch.where((done != 0).all(1), torch.zeros((), dtype=dtype), q_scale * torch_mix(un, hy_tg, embed))
        y = rew.sum(1) + float(np.float32(gamma)) * N
    el = w * QL.element_loss(Qt, y, delta)
    return el.mean(), Qt, y, el, w


def torch_head(inp, dtype, embed, gamma=GAMMA, q_scale=Q_SCALE, delta=0.0, double=True, weight=True, perm=None):
    """The head by torch autograd on the CPU in `dtype` -> dict(g4 = d loss / d y_cur, gh = d loss / d hy_cur, q, td, stats) as float64
    numpy (the statistics computed in `dtype`).  perm: the rows in another order (the per-row outputs come back in the original one)."""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
    if perm is not None:
        t = {k: v[perm] for k, v in t.items()}
    nA = t["rew"].shape[1]
    y_cur, hy_cur = t["y_cur"].clone().requires_grad_(), t["hy_cur"].clone().requires_grad_()
    w = t["weight"][:, 0] if weight else torch.ones_like(t["rew"][:, 0])
    loss, Qt, y, el, w = torch_loss(y_cur, hy_cur, t["y_next_online"], t["y_next_target"], t["hy_next_target"], t["act"], t["rew"], t["done"], w, dtype,
                                    gamma, q_scale, delta, double, embed)
    loss.backward()
    rep = lambda x: x.detach()[:, None].expand(-1, nA)                              # noqa: E731
    out = dict(g4=y_cur.grad, gh=hy_cur.grad, q=rep(Qt), td=rep(y))
    if perm is not None:
        inv = torch.argsort(perm)
        out = {k: v[inv] for k, v in out.items()}
    with torch.no_grad():
        num = lambda x: float(x.double())                                           # noqa: E731
        greedy = (t["act"].argmax(-1) == y_cur.argmax(-1)).to(dtype).mean(1)
        stats = np.array([float(Qt.numel()), num(el.mean()), num(Qt.mean()), num(y.mean()), num((Qt - y).abs().mean()),
                          num((t["done"] != 0).all(1).to(dtype).mean()), num(w.mean()), num(greedy.mean())])
    return dict({k: v.detach().double().numpy() for k, v in out.items()}, stats=stats)


def head_inputs(B, nA, embed, seed=0):
    """CPU tensors {y_cur, y_next_online, y_next_target, act [B, nA, 4], hy_cur, hy_next_target [B, Mh, 4], rew, weight [B, nA]: float32,
    done: uint8}: tanh of normals as both networks' rows, normal scores and rewards, weights uniform in [0.5, 1.5]; done Bernoulli 0.2
    per plane, and every fourth row finished for the whole team.  No value is small enough for a denormal product."""
    g = torch.Generator().manual_seed(8300 + seed + 7 * B + 31 * nA + embed)
    Mh = members(nA, embed)
    rows = lambda n=nA: torch.tanh(torch.randn((B, n, 4), generator=g))           # noqa: E731
    done = torch.rand((B, nA), generator=g) < 0.2
    done[3::4] = True
    return dict(y_cur=rows(), y_next_online=rows(), y_next_target=rows(), hy_cur=rows(Mh), hy_next_target=rows(Mh),
                act=torch.randn((B, nA, 4), generator=g), rew=torch.randn((B, nA), generator=g), done=done.to(torch.uint8),
                weight=torch.rand((B, nA), generator=g) + 0.5)


CORNERS = ("tie in act", "NaN in act", "every plane done, NaN and infinite next rows", "one plane done, its next row NaN", "d = +delta",
           "d = -delta", "pre exactly 0", "pre far below 0", "hypernet values +0 and -0", "NaN d", "tie in y_next", "NaN in y_next_online")
NEEDS_TEAM = (3,)                                   # the corners that need a second plane


def corner_inputs(B, nA, embed, seed=0):
    """head_inputs with batch row r < min(B, len(CORNERS)) rebuilt to hit corner r of the contract -> (inputs, the names that fitted).
    The exact rows use powers of two: with every W1 and w2 at +0 and b1 = 0, pre = 0, h = 0 and tot = b2 = 0.5, so Q_tot = 4 * 0.5 = 2
    EXACTLY; a finished team with rewards summing to 1 (3) makes y = 1 (3) and d = +1 (-1) = +-delta."""
    inp = {k: v.clone() for k, v in head_inputs(B, nA, embed, seed).items()}
    m = embed // 4
    k = nA * m
    row4 = lambda *v: torch.tensor(v, dtype=torch.float32)                         # noqa: E731

    def exact(b, rew):
        inp["done"][b] = 1
        inp["hy_cur"][b] = 0.0
        inp["hy_cur"][b, k + 2 * m, 0] = 0.5
        inp["rew"][b] = 0.0
        inp["rew"][b, 0] = rew
        inp["weight"][b] = 1.0

    def build(r, b):
        if r == 0:
            inp["act"][b] = row4(-1.0, 0.75, 0.75, 0.75)                             # the first maximum: 1
        elif r == 1:
            inp["act"][b] = row4(5.0, -1.0, NAN, 9.0)                                 # a NaN counts as the maximum: 2
        elif r == 2:
            inp["done"][b] = 1
            inp["y_next_target"][b] = NAN
            inp["y_next_online"][b] = row4(INF, -INF, NAN, 1.0)
            inp["hy_next_target"][b] = row4(INF, NAN, -INF, 0.5)
        elif r == 3:
            inp["done"][b] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8)[:nA]
            inp["y_next_target"][b, 0] = NAN                                        # the finished plane's next value stays out of the mix
        elif r == 4:
            exact(b, 1.0)
        elif r == 5:
            exact(b, 3.0)
        elif r == 6:                                                                # pre_e = fmaf(0.5, 0.5, -0.25) = 0 for every e; the others add 0
            inp["act"][b] = row4(0.0, 1.0, 0.0, 0.0)
            inp["y_cur"][b] = row4(0.25, 0.5, -0.5, 0.0)
            inp["hy_cur"][b, :k] = 0.0
            inp["hy_cur"][b, :m] = -0.5                                              # agent 0's W1 = |-0.5|
            inp["hy_cur"][b, k:k + m] = -0.25
        elif r == 7:                                                                # inputs beyond [-1, 1]: pre about -1000 - 50 nA
            inp["hy_cur"][b, k:k + m] = -1000.0
            inp["y_cur"][b] = -50.0
            inp["hy_next_target"][b, k:k + m] = -300.0
        elif r == 8:
            inp["hy_cur"][b, :k] = row4(0.0, -0.0, 0.5, -0.25)
            inp["hy_cur"][b, k + m:k + 2 * m] = row4(-0.0, 0.25, 0.5, 0.0)
            inp["hy_next_target"][b, :k] = row4(-0.0, 0.0, -0.0, 0.0)
        elif r == 9:
            inp["y_cur"][b] = NAN                                                   # u is NaN: pre, Q_tot and d are NaN, clipped or not
        elif r == 10:
            inp["y_next_online"][b] = row4(0.5, 0.5, -0.25, 0.5)
            inp["y_next_target"][b] = row4(-0.5, 0.25, 0.25, 0.0)
            inp["done"][b] = 0
        elif r == 11:
            inp["y_next_online"][b] = row4(0.5, NAN, 0.75, NAN)                       # the FIRST NaN: 1
            inp["y_next_target"][b] = row4(0.9, 0.25, 0.125, -0.5)
            inp["done"][b] = 0
    fitted = []
    for r, name in enumerate(CORNERS):
        if r < B and not (r in NEEDS_TEAM and nA == 1):
            build(r, r)
            fitted.append(name)
    return inp, tuple(fitted)


def _kw(form):
    dbl, delta, w = form
    return dict(delta=delta, double=dbl, weight=w)


@functools.lru_cache(maxsize=None)
def head_case(shape, form, perms=8):
    """(inputs, float64 reference, the float32 yardstick's own error on stats [8] over nine row orders) of a clean case."""
    B, nA, embed = shape
    inp = head_inputs(B, nA, embed)
    ref = ref64(inp, embed, **_kw(form))
    return inp, ref, Y.own_error(lambda order: torch_head(inp, torch.float32, embed, perm=order, **_kw(form)), ref, B, perms)[0]


def head_case_of(shape, form):
    """head_case of a shape of the head suite: at the LARGE_SHAPES with LARGE_PERMS and not kept (one test reads each; a case holds up
    to 400 MB)."""
    return head_case.__wrapped__(shape, form, LARGE_PERMS) if shape in LARGE_SHAPES else head_case(shape, form)


def stats_out_of_bounds(got, ref, e_stats, what=""):
    """n and the mean of `over` (a count: exact in float64) exactly; the others by yardstick_util.scalar_bound."""
    return QL.stats_out_of_bounds(got, ref, e_stats, STAT_NAMES, ((0, "n"), (5, "done")), what)


def guarded_head(inp, embed, form, gamma=GAMMA, q_scale=Q_SCALE, guarded=False, fill=7.0, td=True, keep=None):
    """learner.qmix_head between guard slabs: qlearn_util.guarded_head (its arguments) for this head's outputs and binding."""
    from deep_rl_battlespace_amd import learner as L
    dbl, delta, w = form
    B, nA = inp["rew"].shape
    Mh = members(nA, embed)

    def call(dev, out, ws):
        return L.qmix_head(dev["y_cur"], dev["y_next_target"], dev["hy_cur"], dev["hy_next_target"], dev["act"], dev["rew"], dev["done"], gamma,
                           embed=embed, q_scale=q_scale, y_next_online=dev["y_next_online"] if dbl else None, huber_delta=delta,
                           weight=dev["weight"] if w else None, out=out, workspace=ws)
    return QL.guarded_head(inp, (("g4", (B, nA, 4)), ("gh", (B, Mh, 4)), ("q", (B, nA))), L.qmix_head_workspace_bytes(B, nA), call, guarded, fill,
                           td, keep)


def guarded_inputs(obs, obs_next, Mh, fill=7.0):
    """learner.qmix_inputs between guard slabs -> (x_cur, x_next, the strays)."""
    from deep_rl_battlespace_amd import learner as L
    from guard_util import Buffers
    B, nA, Do = obs.shape
    G = Buffers(True)
    dev = O.put(G, dict(obs=obs, obs_next=obs_next))
    out = tuple(G(k, (B, Mh, nA * Do), torch.float32, init=fill) for k in ("x_cur", "x_next"))
    res = L.qmix_inputs(dev["obs"], dev["obs_next"], Mh, out=out)
    torch.cuda.synchronize()
    assert res[0] is out[0] and res[1] is out[1]
    return out[0], out[1], G.stray()


# ------------------------------------------------------------------------------------------------ a whole update
TEAMS = ((1, 5, 4), (2, 8, 8), (3, 11, 4), (4, 14, 16))            # (nA, Do, embed); the last is the widest mixer: 25 members on 56 inputs
FLOAT64_TEAMS = TEAMS[:3]                                          # (4, 14, 16): 29 networks' kinks per row exceed the cap; bit-for-bit only
B = 64
KW = dict(gamma=GAMMA, tau=0.05, lr=2e-3, max_grad_norm=0.5, q_scale=Q_SCALE, huber_delta=DELTA)
STEP_KW = dict(KW, betas=(0.9, 0.999), eps=1e-3)                    # ddpg_util.STEP_KW's eps, for its reason
KINK = U.KINK                                                       # 1e-4, as dqn_util's
KINK_CAP = 0.25
CASE_SEED = 80
# stepped_case's seed per team, 0 where none is given: the first from 0 at which the float64 reference alone leaves out at most KINK_CAP of
# the rows and no row's arg-max margin lies below KINK (profiles/qmix_float64.json records every seed tried)
STEP_SEEDS = {}


def team_id(team):
    return "nA%d-Do%d-E%d" % team


def make_mixer(nA, Do, embed, seed=0):
    """A mixer on the CPU: mlp_grad_util.make_net "gains" at (Mh, nA Do, 4), head weights scaled to sums of order 1."""
    net = M.make_net(members(nA, embed), nA * Do, 4, "gains", seed + 2)
    with torch.no_grad():
        net.w3.mul_(60.0)
    return net


@functools.lru_cache(maxsize=None)
def learner_case(team, seed=0, batch_size=B):
    """(qnet, mixer, ring rows (N = 4 batch_size; the act rows are score rows), idx of the first batch) of a team.  Read-only."""
    nA, Do, embed = team
    seed += CASE_SEED
    rows = D.ring_rows(4 * batch_size, nA, Do, 4, seed)
    idx = torch.randint(0, 4 * batch_size, (batch_size,), generator=torch.Generator().manual_seed(9500 + seed))
    return Q.make_qnet(nA, Do, seed), make_mixer(nA, Do, embed, seed), rows, idx


def joint(obs, Mh):
    """obs [B, nA, Do] -> the mixer's input [B, Mh, nA Do]: every member reads the row's joint observation."""
    return obs.reshape(obs.shape[0], 1, -1).expand(-1, Mh, -1).contiguous()


def rows_of(nets, batch, dtype, embed):
    """The head's inputs of a batch: the five tanh row tensors evaluated on the CPU in `dtype`.  nets: (qnet, mixer, target qnet, target mixer)."""
    obs, act, rew, obs_next, done = batch
    qnet, mixer, tq, tm = (U._to(n, "cpu", dtype) for n in nets)
    Mh = mixer.n_actors
    with torch.no_grad():
        o, o2 = obs.to(dtype), obs_next.to(dtype)
        return dict(y_cur=qnet(o), y_next_online=qnet(o2), y_next_target=tq(o2), hy_cur=mixer(joint(o, Mh)), hy_next_target=tm(joint(o2, Mh)),
                    act=act.to(dtype), rew=rew.to(dtype), done=done.to(torch.uint8))


def update_reference(nets, batch, w, dtype, embed, double=True, kw=None, perm=None):
    """One whole update on the CPU in `dtype` (float64: the reference; float32: the yardstick) -> dict(g, gm: {tensor: grad} of the Q
    network and of the mixer, net, mix: offpolicy_util.first_step's dicts -- one clip norm per network --, inp: the head's inputs with
    the weights).  nets: (qnet, mixer, target qnet, target mixer); w [B, nA]: column 0 is the row's weight."""
    kw = kw or STEP_KW
    if perm is not None:
        batch, w = tuple(t[perm] for t in batch), w[perm]
    obs, act, rew, obs_next, done = batch
    qnet, mixer, tq, tm = nets
    q, mx, tq_, tm_ = (U._to(n, "cpu", dtype) for n in nets)
    Mh = mixer.n_actors
    o, o2 = obs.to(dtype), obs_next.to(dtype)
    with torch.no_grad():
        y_on, y_tg, hy_tg = q(o2), tq_(o2), tm_(joint(o2, Mh))
    loss = torch_loss(q(o), mx(joint(o, Mh)), y_on, y_tg, hy_tg, act.to(dtype), rew.to(dtype), done.to(torch.uint8), w[:, 0].to(dtype), dtype,
                      kw["gamma"], kw["q_scale"], kw["huber_delta"], double, embed)[0]
    gs = torch.autograd.grad(loss, [getattr(q, p) for p in PARAMS] + [getattr(mx, p) for p in PARAMS])
    g = {p: x.double().numpy() for p, x in zip(PARAMS, gs[:10])}
    gm = {p: x.double().numpy() for p, x in zip(PARAMS, gs[10:])}
    step_q, = O.first_step([qnet], [g], [tq], kw["lr"], kw, dtype)
    step_m, = O.first_step([mixer], [gm], [tm], kw["lr"], kw, dtype)
    return dict(g=g, gm=gm, net=step_q, mix=step_m, inp=dict(rows_of(nets, batch, dtype, embed), weight=w.to(dtype)))


def abs_places(hy, nA, embed):
    """The hypernet values |.| is taken of: W1's and w2's members, as one array [B, (nA m + m) 4]."""
    m = embed // 4
    k = nA * m
    return np.concatenate([hy[:, :k].reshape(hy.shape[0], -1), hy[:, k + m:k + 2 * m].reshape(hy.shape[0], -1)], 1)


def near_kink(nets, batch, ref, embed, kw=None):
    """bool [B, nA], every column the row's: where, in the float64 reference, a hidden unit of the Q network at obs or of the mixer at
    the joint observation lies within KINK of its ReLU's kink, |d| within KINK of the Huber corner, the arg-max margin of the next
    rows below KINK, or a hypernet value that |.| is taken of within KINK of 0."""
    kw = kw or STEP_KW
    qnet, mixer = nets[:2]
    nA = qnet.n_actors
    head = ref64(ref["inp"], embed, kw["gamma"], kw["q_scale"], kw["huber_delta"], True)
    near = U.near_kink((qnet, batch[0])).numpy().any(1)
    near |= U.near_kink((mixer, joint(batch[0], mixer.n_actors))).numpy().any(1)
    near |= np.abs(np.abs(head["q"][:, 0] - head["td"][:, 0]) - kw["huber_delta"]) <= KINK
    near |= (Q.margins(ref["inp"])["y_next"] < KINK).any(1)
    near |= (np.abs(abs_places(ref["inp"]["hy_cur"].double().numpy(), nA, embed)) < KINK).any(1)
    return torch.from_numpy(np.repeat(near[:, None], nA, 1))


def try_seed(team, seed, batch_size=B):
    """(the case or None where it does not qualify, share of rows left out, zeroing rounds, the smallest arg-max margin over ALL rows)."""
    nA, Do, embed = team
    qnet, mixer, rows, idx = learner_case(team, seed, batch_size)
    g = torch.Generator().manual_seed(9700 + seed)
    nets = (qnet, mixer, D.perturbed(qnet, g), D.perturbed(mixer, g))
    batch = tuple(r[idx] for r in rows)
    w0 = (torch.rand((batch_size, 1), generator=g) + 0.5).expand(-1, nA).contiguous()
    ref, w, rounds = O.kink_fixed_point(w0, lambda w: update_reference(nets, batch, w, torch.float64, embed),
                                        lambda ref: near_kink(nets, batch, ref, embed))
    share = float((w == 0).any(1).double().mean())
    m = Q.margins(rows_of(nets, batch, torch.float64, embed))
    low = float(min(m["y_cur"].min(), m["y_next"].min()))
    ok = ref is not None and share <= KINK_CAP and low >= KINK
    case = types.SimpleNamespace(seed=seed, nets=nets, qnet=qnet, mixer=mixer, rows=rows, idx=idx, batch=batch, w=w, rounds=rounds, share=share,
                                 margin=low, ref=ref, embed=embed) if ok else None
    return case, share, rounds, low


@functools.lru_cache(maxsize=None)
def stepped_case(team, batch_size=B):
    """One update from learner_case's networks with targets that are NOT the networks (each parameter plus 0.05 randn), STEP_KW, double Q
    and Huber delta = 1, on the CPU -> a namespace of the starting state, the row weights after the kink filter, ref and yard
    (update_reference in float64 and float32), stats (ref64's) and e_stats (the float32 yardstick's own error over 9 row orders).
    STEP_SEEDS' entry is the team's at B, (team, batch_size)'s elsewhere."""
    c = try_seed(team, STEP_SEEDS.get(team if batch_size == B else (team, batch_size), 0), batch_size)[0]
    assert c is not None, (team, batch_size)
    c.B = batch_size
    kw = STEP_KW
    head = dict(gamma=kw["gamma"], q_scale=kw["q_scale"], delta=kw["huber_delta"], double=True)
    c.yard = update_reference(c.nets, c.batch, c.w, torch.float32, c.embed)
    c.stats = ref64(c.ref["inp"], c.embed, **head)["stats"]
    c.e_stats = Y.own_error(lambda order: torch_head(c.yard["inp"], torch.float32, c.embed, perm=order, **head), dict(stats=c.stats), batch_size)[0]
    return c


# ------------------------------------------------------------------------------------------------ one update by hand
NETS = ("qnet", "mixer")


def snapshot(x):
    """{name: bits} of everything an update of x (a QMIXLearner or a Hand) writes that outlives it: qlearn_util.snapshot of both networks."""
    return QL.snapshot(x, NETS)


class Hand(QL.Hand):
    """What a QMIXLearner holds, under the same names (qlearn_util.Hand), and its update written out with the public primitives alone:
    the ring's sample(), bsx_mlp_forward (offpolicy_util.Hand.forward), qmix_inputs, qmix_head, update_priorities, mlp_grad, mlp_adam_step."""

    def __init__(self, buffer, qnet, mixer, embed=8, q_scale=Q_SCALE, gamma=GAMMA, **kw):
        super().__init__(buffer, dict(qnet=qnet, mixer=mixer), q_scale=q_scale, gamma=gamma, **kw)
        self.embed = embed

    def one(self, obs, act, rew, obs_next, done, u, weight=None, adam=True):
        """The twelve steps on a batch -> (the Q network's gradient row, the mixer's): copies of mlp_grad's cached rows."""
        from deep_rl_battlespace_amd import learner as L
        obs, act, obs_next = obs.contiguous(), act.contiguous(), obs_next.contiguous()
        y_cur, y_on, y_tg = self.q_rows(obs, obs_next)
        x_cur, x_next = L.qmix_inputs(obs, obs_next, self.mixer.n_actors)
        hy_cur, hy_tg = self.forward(self._blob_m, x_cur), self.forward(self._blob_tm, x_next)
        head = L.qmix_head(y_cur, y_tg, hy_cur, hy_tg, act, rew, done, self.gamma, embed=self.embed, q_scale=self.q_scale, y_next_online=y_on,
                           huber_delta=self.huber_delta, weight=weight)
        self.stats[u].copy_(head.stats)
        self.q, self.td = head.q, head.td
        if self.prioritized:
            self.buffer.update_priorities(head.q, head.td)
        row_q = L.mlp_grad(self.qnet, self._blob_q, obs, head.g4, squash=True, input_grad=False)[0].clone()
        row_m = L.mlp_grad(self.mixer, self._blob_m, x_cur, head.gh, squash=True, input_grad=False)[0].clone()
        if adam:
            L.mlp_adam_step([self.qnet], [row_q], [self.adam], [self._blob_q], self.hyper, self.step, targets=[self.target_qnet],
                            target_blobs=[self._blob_tq], stats=self.step_stats[u])
            L.mlp_adam_step([self.mixer], [row_m], [self.adam_mixer], [self._blob_m], self.hyper, self.step_mixer, targets=[self.target_mixer],
                            target_blobs=[self._blob_tm], stats=self.step_stats_mixer[u])
        return row_q, row_m


step_arrays = QL.step_arrays                        # (x, which): "qnet" or "mixer"


def learner_and_hand(team, prioritized=False, rows=None, seed=0, batch_size=B, **kw):
    """(a QMIXLearner, a Hand) of a team on two rings of the same rows and seed, each with its own copies of learner_case's networks."""
    from deep_rl_battlespace_amd import learner as L
    qnet, mixer, case_rows, _ = learner_case(team, seed, batch_size)
    rows = case_rows if rows is None else rows
    kw = {**KW, "embed": team[2], **kw}
    return (L.QMIXLearner(O.ring(rows, batch_size, prioritized=prioritized), O.gpu_copy(qnet), O.gpu_copy(mixer), **kw),
            Hand(O.ring(rows, batch_size, prioritized=prioritized), O.gpu_copy(qnet), O.gpu_copy(mixer), **kw))


# ------------------------------------------------------------------------------------------------ the pay-off VDN cannot fit
# A one-step game: two planes, ONE constant observation per plane, uniform joint actions; the team is paid 1 only when both play action
# 0 (0.5 each), every row finished.  Over the 16 joint actions the least-squares additive fit q1(a) + q2(b) is row mean + column mean -
# grand mean: 7/16 at (0, 0), 3/16 at the six cells with one zero, -1/16 at the nine others; residuals 9/16, -3/16 and 1/16, a mean
# squared error of (81 + 6 * 9 + 9 * 1) / 256 / 16 = 144 / 4096 = 0.03516: VDN's floor (tests/test_qmix_cpu.py solves it numerically).
# Constant observations matter: with random ones a network memorises rows and an additive fit dips below the floor.
TASK = dict(nA=2, Do=5, rows=2048, B=256, lr=2e-3, tau=0.01, q_scale=2.0, huber_delta=0.0, N=600, embeds=(8, 4))
VDN_FLOOR = 144.0 / 4096.0


def task_table():
    """[4, 4] float64: the team's pay-off of every joint action."""
    t = np.zeros((4, 4))
    t[0, 0] = 1.0
    return t


def task_obs(b=TASK):
    """[nA, Do]: the one observation of every plane."""
    return torch.rand((b["nA"], b["Do"]), generator=torch.Generator().manual_seed(9801)) * 2 - 1


def task_rows(seed=0, b=TASK):
    """The ring's rows: the constant observation, random score rows (their arg-max is uniform over the joint actions), 0.5 each where
    both planes' arg-max is 0, every row finished."""
    g = torch.Generator().manual_seed(9800 + seed)
    obs = task_obs(b).expand(b["rows"], -1, -1).contiguous()
    act = torch.randn((b["rows"], b["nA"], 4), generator=g)
    both = (act.argmax(-1) == 0).all(1)
    rew = (0.5 * both.float())[:, None].expand(-1, b["nA"]).contiguous()
    return obs, act, rew, obs.clone(), torch.ones((b["rows"], b["nA"]), dtype=torch.bool)


def task_nets(embed, seed=0, b=TASK):
    """(qnet, mixer) on the CPU, freshly initialised."""
    import actor_ref_util as R
    torch.manual_seed(9850 + seed)
    return R._new(b["nA"], b["Do"], 4), R._new(members(b["nA"], embed), b["nA"] * b["Do"], 4)


def table_of(y4, hy, embed, q_scale):
    """[4, 4] float64: Q_tot of every joint action of two planes from the Q network's rows y4 [2, 4] and the mixer's hy [Mh, 4]."""
    y4, hy = np.asarray(y4, np.float64), np.asarray(hy, np.float64)
    u = np.array([[y4[0, a], y4[1, c]] for a in range(4) for c in range(4)])
    return (q_scale * mix64(u, np.repeat(hy[None], 16, 0), embed)[0]).reshape(4, 4)


def table_error(table):
    """The mean squared error of a Q_tot table over the 16 joint actions."""
    return float(((table - task_table()) ** 2).mean())


def net_table(qnet, mixer, embed, b=TASK):
    """table_of for CPU networks in their own dtype."""
    obs = task_obs(b).to(qnet.w1.dtype)[None]
    with torch.no_grad():
        return table_of(qnet(obs)[0].double().numpy(), mixer(joint(obs, mixer.n_actors))[0].double().numpy(), embed, b["q_scale"])


def task_twin(embed, draws, dtype, seed=0, b=TASK):
    """The torch composition of the learner on the CPU in `dtype`, on the given draws (a list of row-index tensors: one update each):
    autograd through both StackedActors, torch Adam, Polyak targets -> (qnet, mixer, the loss statistic of every update)."""
    rows = task_rows(seed, b)
    qnet, mixer = (U._to(n, "cpu", dtype) for n in task_nets(embed, seed, b))
    tq, tm = copy.deepcopy(qnet), copy.deepcopy(mixer)
    opt = torch.optim.Adam(list(qnet.parameters()) + list(mixer.parameters()), lr=b["lr"])
    Mh, losses = mixer.n_actors, []
    for idx in draws:
        obs, act, rew, obs_next, done = (r[idx] for r in rows)
        o, o2 = obs.to(dtype), obs_next.to(dtype)
        with torch.no_grad():
            y_on, y_tg, hy_tg = qnet(o2), tq(o2), tm(joint(o2, Mh))
        loss = torch_loss(qnet(o), mixer(joint(o, Mh)), y_on, y_tg, hy_tg, act.to(dtype), rew.to(dtype), done.to(torch.uint8),
                          torch.ones(len(idx), dtype=dtype), dtype, GAMMA, b["q_scale"], b["huber_delta"], True, embed)[0]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        O.polyak_((tq, tm), (qnet, mixer), b["tau"])
        losses.append(float(loss.detach().double()))
    return qnet, mixer, losses


def task_draws(N, seed=0, b=TASK):
    """N batches' row indices from a torch generator: what the CPU test feeds the twin (the GPU test feeds it the learner's own draws)."""
    g = torch.Generator().manual_seed(9890 + seed)
    return [torch.randint(0, b["rows"], (b["B"],), generator=g) for _ in range(N)]


# ------------------------------------------------------------------------------------------------ the documented loop
# 64 games of a discrete 2v2 env, T = 8, noise_std = 0.3; NStepAppender(n = 3) into a PrioritizedReplayBuffer of M rows, batches of B
LOOP = dict(n=2, E=64, T=8, M=4096, B=64, nstep=3, iters=3, noise_std=0.3, seed=42, updates=2, embed=8)
