"""What the tests of the DQN head (csrc/bsx_dqn_head.hip: learner.dqn_head) and of DQNLearner share, on top of tests/offpolicy_util.py
and yardstick_util.py:

  argmax4, contract32   the header's contract of bsx_dqn_head restated in numpy float32, operation by operation: g4, q and td are held
                     to it BIT FOR BIT (every operation is specified); fmaf through float64, as offpolicy_util.target32 does it
  ref64              the same contract in float64, statistics included
  torch_head         the head as a torch user writes it -- gather, max, smooth_l1 or mse, autograd from the tanh rows: in float64 the
                     check of the restatement (g4 is d loss / d y4), in float32 the yardstick of the statistics
  head_inputs, corner_inputs, HEAD_SHAPES, FORMS   the head suite's inputs (rounded to float32 once), the rows built to hit the corners
                     of the contract, and its case table
  SPLIT_SHAPES, LARGE_SHAPES, PLANS, LARGE_FORMS, head_cases, split_rows   the shapes at which a VDN row lies across two tiles or
                     workgroups and a workgroup takes J = 2 or 3 tiles, with the plan each must get
  guarded_head       learner.dqn_head with every input, output and the workspace between guard slabs
  TEAMS, learner_case, torch_loss, update_reference, stepped_case   a whole update on the CPU in float64 (the reference) and float32
                     (the yardstick): autograd through StackedActor of the DQN loss, offpolicy_util.first_step as the optimiser step;
                     the row weights leave out what lies near a kink (offpolicy_util.kink_fixed_point): a ReLU's, a Huber corner, an
                     arg-max margin
  Hand, snapshot     one update by hand from the public primitives, holding what a DQNLearner holds under the same names; the bits an
                     update leaves
  the bandit         four arms, the observation's first column decides which of two pays; its torch-composition twin on the learner's
                     own draws, in float64 and float32
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
import mlp_grad_util as M
import offpolicy_util as O
import qlearn_util as QL
import yardstick_util as Y

PARAMS = U.PARAMS
GAMMA = O.GAMMA
Q_SCALE = 4.0                       # a power of two: q_scale * y is exact, which lets a row sit EXACTLY on a Huber corner
DELTA = 1.0
NAN, INF = float("nan"), float("inf")
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dqn_float64.json")
STAT_NAMES = ("loss", "q", "target", "abs_td", "done", "weight", "greedy")          # stats[1..7], learner.DQN_STATS[1:]
# one element; an odd team; one row past a 256-element tile; the widest team
HEAD_SHAPES = ((1, 1), (5, 3), (257, 2), (300, 16))
# (mix, double, huber delta, weighted): both mixes, double on and off, Huber off and delta = 1, weighted and plain
FORMS = tuple((mix, dbl, delta, w) for mix in ("independent", "vdn") for dbl in (True, False) for delta in (0.0, DELTA) for w in (True, False))
# The smallest shapes at which the launch plan (bsx_ddpg_shared.h: plan_of; tiles of TILE elements, at most MAX_BLOCKS workgroups of J
# consecutive tiles) leaves its one-tile-per-workgroup corner, (B, nA) -> (tiles, J, workgroups):
#   SPLIT_SHAPES   a VDN row across two tiles and workgroups: at (171, 3) row 85 is elements 255 .. 257 and row 170 (510 .. 512) ends the
#                  grid; at (103, 5) a 5-agent row lies across tiles 0 and 1.  Every form runs
#   LARGE_SHAPES   J = 2 with split rows at every workgroup edge, two live threads in the last workgroup and one tile past `tiles`;
#                  bsx_td3_head's own (16385, 16), the widest team; J = 3, which tells blockIdx * J from a hard-coded 2.  LARGE_FORMS run:
#                  every template bit takes both values
TILE, MAX_BLOCKS = 256, 1024
SPLIT_SHAPES = ((171, 3), (103, 5))
LARGE_SHAPES = ((87382, 3), (16385, 16), (174763, 3))
PLANS = {(171, 3): (3, 1, 3), (103, 5): (3, 1, 3), (87382, 3): (1025, 2, 513), (16385, 16): (1025, 2, 513), (174763, 3): (2049, 3, 683)}
LARGE_FORMS = (("vdn", True, DELTA, True), ("vdn", False, 0.0, False), ("independent", True, 0.0, True), ("independent", False, DELTA, False))
LARGE_PERMS = 2                     # the yardstick's row orders beside the given one at the LARGE_SHAPES (8 elsewhere): a test stays at seconds


def form_id(form):
    mix, dbl, delta, w = form
    return "%s-%s-%s-%s" % (mix, "double" if dbl else "single", "huber" if delta else "mse", "weighted" if w else "plain")


def shape_id(s):
    return "B%d-nA%d" % s


def head_cases():
    """[(shape, form)] of the head suite: every form at HEAD_SHAPES and SPLIT_SHAPES, LARGE_FORMS at LARGE_SHAPES."""
    return [(s, f) for s in HEAD_SHAPES + SPLIT_SHAPES for f in FORMS] + [(s, f) for s in LARGE_SHAPES for f in LARGE_FORMS]


def head_case_id(c):
    return shape_id(c[0]) + "-" + form_id(c[1])


def split_rows(B, nA):
    """The rows whose nA elements lie in two tiles."""
    b = np.arange(B, dtype=np.int64)
    return np.flatnonzero((b * nA) // TILE != (b * nA + nA - 1) // TILE)


# ------------------------------------------------------------------------------------------------ the head's contract
def argmax4(rows):
    """bsx_argmax4.h's argmax4 over the last axis: the first maximum, a NaN compares as the maximum -- np.argmax's own rule."""
    return np.argmax(rows, -1)


def _take(rows, a):
    return np.take_along_axis(rows, a[..., None], -1)[..., 0]


def _fmaf32(a, x, y):
    """fmaf(a, x, y) of float32 operands: the product is exact in float64 (offpolicy_util.target32's way)."""
    return (np.float64(np.float32(a)) * x.astype(np.float64) + y.astype(np.float64)).astype(np.float32)


def contract32(inp, gamma=GAMMA, q_scale=Q_SCALE, delta=0.0, double=True, mix="independent", weight=True):
    """include/battlespace_hip.h's bsx_dqn_head per element, in numpy float32, every operation rounded once -> dict(g4, q, td)."""
    f = {k: v.numpy() for k, v in inp.items()}
    f32 = np.float32
    B, nA = f["rew"].shape
    qs = f32(q_scale)
    with np.errstate(all="ignore"):
        a = argmax4(f["act"])
        an = argmax4(f["y_next_online"] if double else f["y_next_target"])
        qn = np.where(f["done"] != 0, f32(0.0), qs * _take(f["y_next_target"], an)).astype(f32)
        qc = (qs * _take(f["y_cur"], a)).astype(f32)
        rew = f["rew"].astype(f32)
        if mix == "vdn":
            Q, N, R = qc[:, 0].copy(), qn[:, 0].copy(), rew[:, 0].copy()
            for i in range(1, nA):                                                  # float32 sums in agent order from agent 0
                Q, N, R = (Q + qc[:, i]).astype(f32), (N + qn[:, i]).astype(f32), (R + rew[:, i]).astype(f32)
            Q, N, R = (np.repeat(x[:, None], nA, 1) for x in (Q, N, R))
            w = np.repeat(f["weight"][:, :1], nA, 1) if weight else np.ones((B, nA), f32)
        else:
            Q, N, R = qc, qn, rew
            w = f["weight"] if weight else np.ones((B, nA), f32)
        y, g = QL.tail32(_fmaf32, Q, N, R, w.astype(f32), gamma, q_scale, delta, B)
    g4 = np.zeros((B, nA, 4), f32)
    np.put_along_axis(g4, a[..., None], g[..., None], -1)
    return dict(g4=g4, q=Q.astype(f32), td=y)


def ref64(inp, gamma=GAMMA, q_scale=Q_SCALE, delta=0.0, double=True, mix="independent", weight=True):
    """The same contract in float64 numpy on the inputs as given -> dict(g4, q, td, stats [8])."""
    f = {k: (v.double().numpy() if v.is_floating_point() else v.numpy()) for k, v in inp.items()}
    B, nA = f["rew"].shape
    gamma = float(np.float32(gamma))
    with np.errstate(all="ignore"):
        a = argmax4(f["act"])
        an = argmax4(f["y_next_online"] if double else f["y_next_target"])
        over = f["done"] != 0
        qn = np.where(over, 0.0, q_scale * _take(f["y_next_target"], an))
        qc = q_scale * _take(f["y_cur"], a)
        w = f["weight"] if weight else np.ones((B, nA))
        Q, N, R = qc, qn, f["rew"]
        if mix == "vdn":
            Q, N, R = (np.repeat(x.sum(1, keepdims=True), nA, 1) for x in (qc, qn, f["rew"]))
            w = np.repeat(w[:, :1], nA, 1)
        y, d, loss, g = QL.tail64(Q, N, R, w, gamma, q_scale, delta, B)
        g4 = np.zeros((B, nA, 4))
        np.put_along_axis(g4, a[..., None], g[..., None], -1)
        stats = QL.stats64(float(B * nA), w, loss, Q, y, d, over, a == argmax4(f["y_cur"]))
    return dict(g4=g4, q=Q, td=y, stats=stats)


def torch_loss(y_cur, y_on, y_tg, act, rew, done, w, dtype, gamma, q_scale, delta, double, mix):
    """The DQN loss as a torch user writes it from the three tanh row tensors -> (loss, Q, y, per-element w l(d), w), Q, y and w
    [B, nA].  independent: sum_i mean_b w l(Q_i - y_i); vdn: mean_b w[:, 0] l(Q_tot - y_tot).  l = mse, or 2 delta smooth_l1(beta=delta)."""
    a = act.argmax(-1, keepdim=True)
    Q = q_scale * y_cur.gather(-1, a)[..., 0]
    with torch.no_grad():
        nxt = y_tg.gather(-1, y_on.argmax(-1, keepdim=True))[..., 0] if double else y_tg.max(-1).values
        N, R = (1.0 - done.to(dtype)) * q_scale * nxt, rew
        if mix == "vdn":
            N, R, w = N.sum(1, keepdim=True), R.sum(1, keepdim=True), w[:, :1]
        y = R + float(np.float32(gamma)) * N
    if mix == "vdn":
        Q = Q.sum(1, keepdim=True)
    el = w * QL.element_loss(Q, y, delta)
    nA = act.shape[1]
    full = lambda x: x.expand(-1, nA)                                               # noqa: E731
    return el.mean(0).sum(), full(Q), full(y), full(el), full(w)


def torch_head(inp, dtype, gamma=GAMMA, q_scale=Q_SCALE, delta=0.0, double=True, mix="independent", weight=True, perm=None):
    """The head by torch autograd on the CPU in `dtype` -> dict(g4 = d loss / d y_cur, q, td, stats) as float64 numpy (the statistics
    computed in `dtype`).  perm: the rows in another order (the per-row outputs come back in the original one)."""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
    if perm is not None:
        t = {k: v[perm] for k, v in t.items()}
    y_cur = t["y_cur"].clone().requires_grad_()
    w = t["weight"] if weight else torch.ones_like(t["rew"])
    loss, Q, y, el, w = torch_loss(y_cur, t["y_next_online"], t["y_next_target"], t["act"], t["rew"], t["done"], w, dtype, gamma, q_scale, delta,
                                   double, mix)
    loss.backward()
    out = dict(g4=y_cur.grad, q=Q.detach(), td=y)
    if perm is not None:
        inv = torch.argsort(perm)
        out = {k: v[inv] for k, v in out.items()}
    with torch.no_grad():
        num = lambda x: float(x.double())                                           # noqa: E731
        greedy = (t["act"].argmax(-1) == y_cur.argmax(-1)).to(dtype)
        stats = np.array([float(Q.numel()), num(el.mean()), num(Q.mean()), num(y.mean()), num((Q - y).abs().mean()),
                          num(t["done"].to(dtype).mean()), num(w.mean()), num(greedy.mean())])
    return dict({k: v.detach().double().numpy() for k, v in out.items()}, stats=stats)


def head_inputs(B, nA, seed=0):
    """{y_cur, y_next_online, y_next_target, act [B, nA, 4], rew, weight [B, nA]: float32, done: uint8} CPU tensors: tanh of normals as
    the rows, normal scores and rewards, done Bernoulli 0.2, weights uniform in [0.5, 1.5].  With Q_SCALE = 4 and DELTA = 1 about
    a third of the elements lie inside the Huber corner."""
    g = torch.Generator().manual_seed(8100 + seed + 7 * B + nA)
    rows = lambda: torch.tanh(torch.randn((B, nA, 4), generator=g))               # noqa: E731
    return dict(y_cur=rows(), y_next_online=rows(), y_next_target=rows(), act=torch.randn((B, nA, 4), generator=g),
                rew=torch.randn((B, nA), generator=g), done=(torch.rand((B, nA), generator=g) < 0.2).to(torch.uint8),
                weight=torch.rand((B, nA), generator=g) + 0.5)


CORNERS = ("tie in act", "tie in y_next", "tie in y_cur", "NaN in act", "NaN in y_next_online", "done with NaN next", "done with inf next",
           "NaN d", "d = +delta", "d = -delta", "one agent done, the next not", "all four scores equal")


def corner_inputs(B, nA, seed=0):
    """head_inputs with batch row r < min(B, len(CORNERS)) rebuilt to hit corner r of the contract (all agents of the row alike unless
    said) -> (inputs, the names of the corners that fitted).  Q_SCALE a power of two and done rows make |d| EXACTLY delta:
    Q = 4 * 0.5, y = fmaf(gamma, 0, 1) = 1 (agent 0; the row's other agents contribute exact zeros, so the VDN sums hit it too)."""
    inp = {k: v.clone() for k, v in head_inputs(B, nA, seed).items()}
    row4 = lambda *v: torch.tensor(v, dtype=torch.float32)                         # noqa: E731

    def exact(b, rew):                                                              # a finished row whose d is (2 - rew) at agent 0
        inp["done"][b] = 1
        inp["act"][b] = row4(0.0, 1.0, 0.0, 0.0)
        inp["y_cur"][b] = 0.0
        inp["y_cur"][b, 0] = row4(0.25, 0.5, -0.5, 0.0)
        inp["rew"][b] = 0.0
        inp["rew"][b, 0] = rew
        inp["weight"][b] = 1.0

    def build(r, b):
        if r == 0:
            inp["act"][b] = row4(-1.0, 0.75, 0.75, 0.75)                             # the first maximum: 1
        elif r == 1:
            inp["y_next_online"][b] = row4(0.5, 0.5, -0.25, 0.5)
            inp["y_next_target"][b] = row4(-0.5, 0.25, 0.25, 0.0)
            inp["done"][b] = 0
        elif r == 2:
            inp["y_cur"][b] = row4(0.125, 0.875, 0.875, -1.0)
        elif r == 3:
            inp["act"][b] = row4(5.0, -1.0, NAN, 9.0)                                 # a NaN counts as the maximum: 2
        elif r == 4:
            inp["y_next_online"][b] = row4(0.5, NAN, 0.75, NAN)                       # ... and the FIRST NaN: 1
            inp["y_next_target"][b] = row4(0.9, 0.25, NAN, -0.5)
            inp["done"][b] = 0
        elif r == 5:
            inp["done"][b] = 1
            inp["y_next_target"][b] = NAN
            inp["y_next_online"][b] = NAN
        elif r == 6:
            inp["done"][b] = 1
            inp["y_next_target"][b] = row4(INF, -INF, INF, 1.0)
        elif r == 7:
            inp["y_cur"][b] = NAN                                                   # Q is NaN: d is NaN, clipped or not
        elif r == 8:
            exact(b, 1.0)
        elif r == 9:
            exact(b, 3.0)
        elif r == 10 and nA > 1:
            inp["done"][b] = torch.tensor([1, 0] * nA, dtype=torch.uint8)[:nA]
            inp["y_next_target"][b, 0] = NAN                                        # the finished agent's next value stays out of the sum
        elif r == 11:
            inp["act"][b] = 0.25
            inp["y_cur"][b] = -0.5
            inp["y_next_online"][b] = 1.0
    fitted = []
    for r, name in enumerate(CORNERS):
        if r < B and not (r == 10 and nA == 1):
            build(r, r)
            fitted.append(name)
    return inp, tuple(fitted)


def same_bits_or_nan(got, want):
    """got, want: float32 arrays -> whether they hold the same bits wherever `want` is a number and a NaN wherever it is a NaN (the
    contract says a NaN stays a NaN, not which one: a processor's default NaN has its own sign and payload)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


@functools.lru_cache(maxsize=None)
def head_case(B, nA, form, perms=8):
    """(inputs, float64 reference, float32 yardstick, the yardstick's own error on stats [8] over nine row orders) of a clean case."""
    mix, dbl, delta, w = form
    kw = dict(delta=delta, double=dbl, mix=mix, weight=w)
    inp = head_inputs(B, nA)
    ref = ref64(inp, **kw)
    yard = torch_head(inp, torch.float32, **kw)
    return inp, ref, yard, Y.own_error(lambda order: torch_head(inp, torch.float32, perm=order, **kw), ref, B, perms)[0]


def head_case_of(BnA, form):
    """head_case of a shape of the head suite: at the LARGE_SHAPES with LARGE_PERMS and not kept (one test reads each)."""
    return head_case.__wrapped__(*BnA, form, LARGE_PERMS) if BnA in LARGE_SHAPES else head_case(*BnA, form)


def stats_out_of_bounds(got, ref, e_stats, what=""):
    """n and the two counts' means (done, greedy: exact in float64) exactly; the others by yardstick_util.scalar_bound."""
    return QL.stats_out_of_bounds(got, ref, e_stats, STAT_NAMES, ((0, "n"), (5, "done"), (7, "greedy")), what)


def guarded_head(inp, form, gamma=GAMMA, q_scale=Q_SCALE, guarded=False, fill=7.0, td=True, keep=None):
    """learner.dqn_head between guard slabs: qlearn_util.guarded_head (its arguments) for this head's outputs and binding."""
    from deep_rl_battlespace_amd import learner as L
    mix, dbl, delta, w = form
    B, nA = inp["rew"].shape

    def call(dev, out, ws):
        return L.dqn_head(dev["y_cur"], dev["y_next_target"], dev["act"], dev["rew"], dev["done"], gamma, q_scale=q_scale,
                          y_next_online=dev["y_next_online"] if dbl else None, mix=mix, huber_delta=delta, weight=dev["weight"] if w else None,
                          out=out, workspace=ws)
    return QL.guarded_head(inp, (("g4", (B, nA, 4)), ("q", (B, nA))), L.dqn_head_workspace_bytes(B, nA), call, guarded, fill, td, keep)


# ------------------------------------------------------------------------------------------------ a whole update
TEAMS = ((1, 5), (2, 8), (3, 11), (16, 50))         # (nA, Do)
B = 64
B_SPLIT = SPLIT_SHAPES[0][0]                        # 171 rows of a 3v3 team: three tiles, the VDN rows 85 and 170 split (SPLIT_SHAPES)
MIXES = ("independent", "vdn")
# (team, mix, batch) of the whole-update cases against float64: every team with both mixes at B, and the 3v3 team above one tile
STEP_CASES = tuple((t, m, B) for t in TEAMS for m in MIXES) + tuple((TEAMS[2], m, B_SPLIT) for m in MIXES)
KW = dict(gamma=GAMMA, tau=0.05, lr=2e-3, max_grad_norm=0.5, q_scale=Q_SCALE, huber_delta=DELTA)
# ddpg_util.STEP_KW's eps, for its reason: at eps = 1e-8 Adam's first step is lr sign(g) and a gradient error of float32's size moves a parameter by lr
STEP_KW = dict(KW, betas=(0.9, 0.999), eps=1e-3)
KINK = U.KINK                                       # 1e-4: a ReLU's kink, a Huber corner and an arg-max margin alike -- a hundred
#                                                     times what float32 loses on a tanh row (about 1e-6) or on d (about 4e-6)
KINK_CAP = 0.25                                     # at most a quarter of the rows may be filtered
CASE_SEED = 60
# stepped_case's seed per (team, mix), 0 where none is given: the first seed from 0 at which the float64 reference alone leaves out at
# most KINK_CAP of the rows and no row's arg-max margin lies below KINK (profiles/dqn_float64.json records every seed tried)
STEP_SEEDS = {}


def step_seed(team, mix, batch_size=B):
    """STEP_SEEDS' entry of a case: under (team, mix) at B, under (team, mix, batch_size) elsewhere."""
    return STEP_SEEDS.get((team, mix) if batch_size == B else (team, mix, batch_size), 0)


def team_id(team, mix=None, batch_size=B):
    return "nA%d-Do%d" % team + ("" if mix is None else "-" + mix) + ("" if batch_size == B else "-B%d" % batch_size)


def make_qnet(nA, Do, seed=0):
    """A Q network on the CPU: mlp_grad_util.make_net "gains", head weights scaled to sums of order 1 (ddpg_util.make_nets' actor)."""
    net = M.make_net(nA, Do, 4, "gains", seed + 1)
    with torch.no_grad():
        net.w3.mul_(60.0)
    return net


@functools.lru_cache(maxsize=None)
def learner_case(team, seed=0, batch_size=B):
    """(qnet, ring rows (N = 4 batch_size; the act rows are score rows), idx of the first batch) of a team.  Read-only."""
    nA, Do = team
    seed += CASE_SEED
    qnet = make_qnet(nA, Do, seed)
    rows = D.ring_rows(4 * batch_size, nA, Do, 4, seed)
    idx = torch.randint(0, 4 * batch_size, (batch_size,), generator=torch.Generator().manual_seed(9500 + seed))
    return qnet, rows, idx


def rows_of(qnet, target, batch, dtype):
    """The head's inputs of a batch: the three tanh row tensors evaluated on the CPU in `dtype`."""
    obs, act, rew, obs_next, done = batch
    to = lambda n: U._to(n, "cpu", dtype)                                           # noqa: E731
    with torch.no_grad():
        o, o2 = obs.to(dtype), obs_next.to(dtype)
        return dict(y_cur=to(qnet)(o), y_next_online=to(qnet)(o2), y_next_target=to(target)(o2), act=act.to(dtype), rew=rew.to(dtype),
                    done=done.to(torch.uint8))


def update_reference(qnet, target, batch, w, dtype, mix, double=True, kw=None, perm=None):
    """One whole update on the CPU in `dtype` (float64: the reference; float32: the yardstick) -> dict(g: {tensor: grad}, net:
    offpolicy_util.first_step's dict, inp: the head's inputs with the weights).  perm: the batch's rows in another order."""
    kw = kw or STEP_KW
    if perm is not None:
        batch, w = tuple(t[perm] for t in batch), w[perm]
    obs, act, rew, obs_next, done = batch
    q, tg = U._to(qnet, "cpu", dtype), U._to(target, "cpu", dtype)
    o, o2 = obs.to(dtype), obs_next.to(dtype)
    with torch.no_grad():
        y_on, y_tg = q(o2), tg(o2)
    loss = torch_loss(q(o), y_on, y_tg, act.to(dtype), rew.to(dtype), done, w.to(dtype), dtype, kw["gamma"], kw["q_scale"], kw["huber_delta"],
                      double, mix)[0]
    gs = torch.autograd.grad(loss, [getattr(q, p) for p in PARAMS])
    g = {p: x.double().numpy() for p, x in zip(PARAMS, gs)}
    step, = O.first_step([qnet], [g], [target], kw["lr"], kw, dtype)
    return dict(g=g, net=step, inp=dict(rows_of(qnet, target, batch, dtype), weight=w.to(dtype)))


def margins(inp, double=True):
    """{name: [B, nA] float64}: the gap between the two largest scores of the rows an arg-max is taken of."""
    top = lambda x: (lambda s: s[..., 3] - s[..., 2])(np.sort(x.double().numpy(), -1))      # noqa: E731
    return dict(y_cur=top(inp["y_cur"]), y_next=top(inp["y_next_online" if double else "y_next_target"]), act=top(inp["act"]))


def near_kink(qnet, batch, ref, mix, kw=None):
    """bool [B, nA]: where, in the float64 reference, a hidden unit of the Q network at obs lies within KINK of its ReLU's kink, |d| within
    KINK of the Huber corner, or the arg-max margin of the next rows below KINK.  Under VDN a row has ONE weight: any agent's kink is
    the row's."""
    kw = kw or STEP_KW
    head = ref64(ref["inp"], kw["gamma"], kw["q_scale"], kw["huber_delta"], True, mix)
    near = U.near_kink((qnet, batch[0])).numpy()
    near |= np.abs(np.abs(head["q"] - head["td"]) - kw["huber_delta"]) <= KINK
    near |= margins(ref["inp"])["y_next"] < KINK
    if mix == "vdn":
        near = np.repeat(near.any(1, keepdims=True), near.shape[1], 1)
    return torch.from_numpy(near)


def try_seed(team, mix, seed, batch_size=B):
    """(the case or None where it does not qualify, share of rows left out, zeroing rounds, the smallest arg-max margin over ALL rows)."""
    qnet, rows, idx = learner_case(team, seed, batch_size)
    g = torch.Generator().manual_seed(9700 + seed)
    target = D.perturbed(qnet, g)
    batch = tuple(r[idx] for r in rows)
    w0 = torch.rand((batch_size, team[0]), generator=g) + 0.5
    ref, w, rounds = O.kink_fixed_point(w0, lambda w: update_reference(qnet, target, batch, w, torch.float64, mix),
                                        lambda ref: near_kink(qnet, batch, ref, mix))
    share = float((w == 0).any(1).double().mean())
    m = margins(rows_of(qnet, target, batch, torch.float64))
    low = float(min(m["y_cur"].min(), m["y_next"].min()))
    ok = ref is not None and share <= KINK_CAP and low >= KINK
    case = types.SimpleNamespace(seed=seed, qnet=qnet, target=target, rows=rows, idx=idx, batch=batch, w=w, rounds=rounds, share=share,
                                 margin=low, ref=ref) if ok else None
    return case, share, rounds, low


@functools.lru_cache(maxsize=None)
def stepped_case(team, mix, batch_size=B):
    """One update from learner_case's network with a target that is NOT the network (each parameter plus 0.05 randn), STEP_KW, double Q
    and Huber delta = 1, on the CPU -> a namespace of the starting state, the row weights after the kink filter, ref and yard
    (update_reference in float64 and float32), stats (ref64's) and e_stats (the float32 yardstick's own error over 9 row orders)."""
    c = try_seed(team, mix, step_seed(team, mix, batch_size), batch_size)[0]
    assert c is not None, (team, mix, batch_size)
    c.B = batch_size
    kw = STEP_KW
    head = dict(gamma=kw["gamma"], q_scale=kw["q_scale"], delta=kw["huber_delta"], double=True, mix=mix)
    c.yard = update_reference(c.qnet, c.target, c.batch, c.w, torch.float32, mix)
    c.stats = ref64(c.ref["inp"], **head)["stats"]
    c.e_stats = Y.own_error(lambda order: torch_head(c.yard["inp"], torch.float32, perm=order, **head), dict(stats=c.stats), batch_size)[0]
    return c


# ------------------------------------------------------------------------------------------------ one update by hand
snapshot, step_arrays = QL.snapshot, QL.step_arrays     # of the one network "qnet": the defaults


class Hand(QL.Hand):
    """What a DQNLearner holds, under the same names (qlearn_util.Hand), and its update written out with the public primitives alone:
    the ring's sample(), bsx_mlp_forward (offpolicy_util.Hand.forward), dqn_head, update_priorities, mlp_grad, mlp_adam_step."""

    def __init__(self, buffer, qnet, mix="independent", q_scale=Q_SCALE, gamma=GAMMA, **kw):
        super().__init__(buffer, dict(qnet=qnet), q_scale=q_scale, gamma=gamma, **kw)
        self.mix = mix

    def one(self, obs, act, rew, obs_next, done, u, weight=None, adam=True):
        """The seven steps on a batch -> the network's gradient row (a copy of mlp_grad's cached row)."""
        from deep_rl_battlespace_amd import learner as L
        obs, act, obs_next = obs.contiguous(), act.contiguous(), obs_next.contiguous()
        y_cur, y_on, y_tg = self.q_rows(obs, obs_next)
        head = L.dqn_head(y_cur, y_tg, act, rew, done, self.gamma, q_scale=self.q_scale, y_next_online=y_on, mix=self.mix,
                          huber_delta=self.huber_delta, weight=weight)
        self.stats[u].copy_(head.stats)
        self.q, self.td = head.q, head.td
        if self.prioritized:
            self.buffer.update_priorities(head.q, head.td)
        row = L.mlp_grad(self.qnet, self._blob_q, obs, head.g4, squash=True, input_grad=False)[0].clone()
        if adam:
            L.mlp_adam_step([self.qnet], [row], [self.adam], [self._blob_q], self.hyper, self.step, targets=[self.target_qnet],
                            target_blobs=[self._blob_tq], stats=self.step_stats[u])
        return row


def learner_and_hand(team, prioritized=False, rows=None, seed=0, batch_size=B, **kw):
    """(a DQNLearner, a Hand) of a team on two rings of the same rows and seed, each with its own copy of learner_case's network."""
    from deep_rl_battlespace_amd import learner as L
    qnet, case_rows, _ = learner_case(team, seed, batch_size)
    rows = case_rows if rows is None else rows
    kw = {**KW, **kw}
    return (L.DQNLearner(O.ring(rows, batch_size, prioritized=prioritized), O.gpu_copy(qnet), **kw),
            Hand(O.ring(rows, batch_size, prioritized=prioritized), O.gpu_copy(qnet), **kw))


# ------------------------------------------------------------------------------------------------ the bandit
# Four arms; the observation's first column decides which of two pays 1 (arm 1 where it is positive, arm 3 where not), every other arm 0.
# One-step rows (done = 1): Q's fixed point is the reward itself, in [0, 1] <= q_scale = 2.  N and MARGIN were chosen with the float32
# torch composition ALONE, on the CPU (tests/test_dqn_cpu.py re-runs it): N the smallest of 100, 200, 300, 400 (it is the first) after which its greedy
# action is the paying arm on every probe observation with |o_0| >= MARGIN, for both mixes.
BANDIT = dict(nA=2, Do=5, rows=2048, B=256, probes=512, lr=2e-3, tau=0.01, q_scale=2.0, huber_delta=1.0, N=100, MARGIN=0.1)


def bandit_best(obs):
    """[.., nA] int64: the arm that pays."""
    return torch.where(obs[..., 0] > 0, 1, 3)


def bandit_rows(seed=0, b=BANDIT):
    """(the bandit ring's rows: uniform observations, random score rows, reward 1 where the row's arg-max is the paying arm, every row
    finished; the probe observations, |o_0| >= MARGIN)."""
    g = torch.Generator().manual_seed(9900 + seed)
    uni = lambda *s: torch.rand(s, generator=g) * 2 - 1                            # noqa: E731
    obs, act = uni(b["rows"], b["nA"], b["Do"]), torch.randn((b["rows"], b["nA"], 4), generator=g)
    rew = (act.argmax(-1) == bandit_best(obs)).float()
    rows = (obs, act, rew, uni(b["rows"], b["nA"], b["Do"]), torch.ones((b["rows"], b["nA"]), dtype=torch.bool))
    probe = uni(b["probes"], b["nA"], b["Do"])
    probe[..., 0] = torch.where(probe[..., 0].abs() < b["MARGIN"], torch.sign(probe[..., 0] + 1e-9) * b["MARGIN"], probe[..., 0])
    return rows, probe


def bandit_qnet(seed=0, b=BANDIT):
    torch.manual_seed(9950 + seed)
    import actor_ref_util as R
    return R._new(b["nA"], b["Do"], 4)


def bandit_twin(mix, draws, dtype, seed=0, b=BANDIT):
    """The torch composition of the learner on the CPU in `dtype`, on the given draws (a list of row-index tensors: one update each):
    autograd through StackedActor, torch Adam, foreach Polyak -> (the network, the loss statistic of every update: mean over the
    B nA elements of w l(d), w = 1)."""
    rows, _ = bandit_rows(seed, b)
    net = U._to(bandit_qnet(seed, b), "cpu", dtype)
    target = copy.deepcopy(net)
    opt = torch.optim.Adam(net.parameters(), lr=b["lr"])
    losses = []
    for idx in draws:
        obs, act, rew, obs_next, done = (r[idx] for r in rows)
        o, o2 = obs.to(dtype), obs_next.to(dtype)
        with torch.no_grad():
            y_on, y_tg = net(o2), target(o2)
        loss, _, _, el, _ = torch_loss(net(o), y_on, y_tg, act.to(dtype), rew.to(dtype), done, torch.ones_like(rew, dtype=dtype), dtype, GAMMA,
                                       b["q_scale"], b["huber_delta"], True, mix)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        O.polyak_((target,), (net,), b["tau"])
        losses.append(float(el.detach().double().mean()))
    return net, losses


def bandit_draws(N, seed=0, b=BANDIT):
    """N batches' row indices from a torch generator: what the CPU test feeds the twin (the GPU test feeds it the learner's own draws)."""
    g = torch.Generator().manual_seed(9990 + seed)
    return [torch.randint(0, b["rows"], (b["B"],), generator=g) for _ in range(N)]


def greedy_is_best(net, probe):
    with torch.no_grad():
        return bool((net(probe.to(net.w1.dtype)).argmax(-1) == bandit_best(probe)).all())


# ------------------------------------------------------------------------------------------------ the documented loop
# 64 games of a discrete 2v2 env, T = 8, noise_std = 0.3; NStepAppender(n = 3) into a PrioritizedReplayBuffer of M rows, batches of B
LOOP = dict(n=2, E=64, T=8, M=4096, B=64, nstep=3, iters=3, noise_std=0.3, seed=42, updates=2, mixes=MIXES)
