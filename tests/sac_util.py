"""What the tests of the SAC kernels (csrc/bsx_sac_head.hip: learner.sac_sample_actions, sac_head, sac_policy_seed, sac_policy_grad) and of
SACLearner share, on top of tests/td3_util.py and tests/ddpg_util.py (the shapes, the joins, the learner's case, the joint step, the
bandit), yardstick_util (the bars), philox_util (normals4), adam_util / adam_mlp_util (the float64 steps) and guard_util:

  gauss, ref_sample, torch_sample      the reparameterised draw and its log-probability: the contract in numpy (any dtype), x after the
                           call, and the draw as a torch user writes it
  sac_inputs, ref_sac_head, torch_sac, sac_case, contract32, head_spread, factors, check_sac   the soft twin head: its inputs, its contract
                           in float64 numpy, the head as a torch user writes it with autograd, cached per shape, and the bounds
  ref_policy_seed, policy_inputs, ref_policy_grad, torch_policy_grad, policy_case, ga32   the seeds bit for bit; sac_policy_grad's contract
                           in float64, as a torch user writes it in float32, and g_a4's float32 restatement
  losses                   L_critic, L_pi and L_alpha as the issue writes them, under torch autograd in any dtype
  Hand, snapshot, blobs_are_packs   one SAC update by hand from the public primitives, holding what a SACLearner holds under the same names
  sac_grads, update_reference, stepped_case, wrong_variants   a whole update in float64 and float32 on the CPU with injected normals
  torch_update, bandit_rows, bandit_nets, bandit_torch_run   the torch composition of the same SAC and what it reaches on the bandit at k = 3

Nothing here imports the native library at import time."""
import copy
import functools
import math
import os
import types

import numpy as np
import torch

import ddpg_util as D
import guard_util as G                # noqa: F401  (the suites take Buffers from here)
import philox_util as PU
import td3_util as T
import yardstick_util as Y

AU, AM, U, R, PARAMS = D.AU, T.AM, D.U, D.R, D.PARAMS
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sac_float64.json")
SALT = 0x60000000                                                   # include/battlespace_hip.h: BSX_SAC_SALT
OTHER_SALTS = T.OTHER_SALTS + (T.SALT,)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
TARGET_ENTROPY = -3.0
HEAD_SHAPES = T.HEAD_SHAPES
K3 = tuple(dict.fromkeys((B, nA, Do, 3, c) for B, nA, Do, _, c in D.SHAPES))                   # ddpg_util.SHAPES with k = 3
SAMPLE_SHAPES = K3
GRAD_SHAPES = tuple(dict.fromkeys((B, nA, Do, 3, c) for B, nA, Do, _, _ in D.SHAPES[:-1] for c in (0, 1)
                                  if D.width(nA, Do, 3, c) <= 64)) + ((16385, 16, 1, 3, 0),)
HAND_SHAPES = ((161, 2, 8, 3, 1), (97, 1, 5, 3, 0), (129, 3, 11, 3, 1), (1, 1, 5, 3, 1))
MAIN_SHAPES = HAND_SHAPES[:2]
TD_NAMES = ("g_q1", "g_q2", "td")
STAT_NAMES = T.STAT_NAMES
PI_STAT_NAMES = ("actor_loss", "q_pi", "logp", "alpha", "weight", "picked_1")       # stats_pi[1..6]
# stepped_case's seed per shape: the first from 0 at which, on the float64 reference alone, the kink filter closes within
# ddpg_util.MAX_ROUNDS zeroing rounds and leaves out less than actor_grad_util.KINK_CAP.  profiles/sac_float64.json records what every
# seed tried gave
STEP_SEEDS = {}
if os.path.exists(PROFILE):
    import json
    STEP_SEEDS = {tuple(v["shape"]): v["seed"] for v in json.load(open(PROFILE)).get("stepped", {}).get("cases", {}).values()}


# ------------------------------------------------------------------------------------------------ the draw
def gauss(y4, log_std, z):
    """(a [B, nA, 3], logp [B, nA]) of the header's contract in y4's dtype (float64: the reference)."""
    t = y4.dtype.type
    l, zz = log_std.astype(y4.dtype)[None], z.astype(y4.dtype)[..., :3]
    with np.errstate(all="ignore"):
        a = np.exp(l) * zz + y4[..., :3]
        q = (t(-0.5) * zz) * zz - l
    return a.astype(y4.dtype), (((q[..., 0] + q[..., 1]) + q[..., 2]) - t(3.0) * t(HALF_LOG_2PI)).astype(y4.dtype)


def ref_sample(y4, log_std, z, x, Do, central, own_only):
    """bsx_sac_sample_actions with injected normals in y4's dtype -> (a new x, logp)."""
    a, logp = gauss(y4, log_std, z)
    a4 = np.concatenate([a, np.zeros((*a.shape[:2], 1), a.dtype)], -1)
    return D.ref_put_actions(a4, x.astype(y4.dtype), Do, 3, central, own_only), logp


def torch_sample(y4, log_std, z, dtype=torch.float32):
    """The draw as a torch user writes it (rollout.gaussian_log_prob's expression) -> (a, logp) as float64 numpy."""
    mu, l, zz = torch.from_numpy(y4).to(dtype)[..., :3], torch.from_numpy(log_std).to(dtype), torch.from_numpy(z).to(dtype)[..., :3]
    a = mu + torch.exp(l) * zz
    logp = (-0.5 * zz * zz - l).sum(-1) - 1.5 * math.log(2.0 * math.pi)
    return a.double().numpy(), logp.double().numpy()


def philox_normals(seed, seq, B, nA):
    """normals4(seed, seq, b nA + j, SALT) -> float64 [B, nA, 4]."""
    return PU.normals4(seed, seq, np.arange(B * nA, dtype=np.uint64), SALT).reshape(B, nA, 4)


def sample_arrays(shape, seed=0):
    """(y4, log_std, z) float32 numpy: tanh rows, log_std about -1, standard normals."""
    B, nA = shape[:2]
    g = np.random.default_rng(41 + seed)
    return (np.tanh(2.0 * g.standard_normal((B, nA, 4))).astype(np.float32), (-1.0 + 0.3 * g.standard_normal((nA, 3))).astype(np.float32),
            g.standard_normal((B, nA, 4)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the soft twin head
def sac_inputs(B, nA, seed=0):
    """td3_util.td3_inputs' tensors, logp_next = randn - 1 and log_alpha = log 0.2 + 0.3 randn [nA]."""
    g = torch.Generator().manual_seed(8700 + seed + 7 * B + nA)
    return dict(T.td3_inputs(B, nA, seed), logp_next=torch.randn((B, nA), generator=g) - 1.0,
                log_alpha=math.log(0.2) + 0.3 * torch.randn((nA,), generator=g))


def ref_sac_head(inp, gamma=D.GAMMA, weight=True):
    """The contract in float64 numpy -> dict(g_q1, g_q2 [B, nA, 4], td [B, nA], stats [8])."""
    f = {k: v.double().numpy() for k, v in inp.items()}
    B, nA = f["q1"].shape
    over = f["done"] != 0
    w = f["weight"] if weight else np.ones((B, nA))
    with np.errstate(all="ignore"):
        v = np.minimum(f["q1_next"], f["q2_next"]) - np.exp(f["log_alpha"])[None] * f["logp_next"]
        y = gamma * np.where(over, 0.0, v) + f["rew"]
    d1, d2 = f["q1"] - y, f["q2"] - y
    out = {k: np.zeros((B, nA, 4)) for k in ("g_q1", "g_q2")}
    out["g_q1"][..., 0], out["g_q2"][..., 0] = w * d1 * (2.0 / B), w * d2 * (2.0 / B)
    n = float(B * nA)
    stats = np.array([n, (w * (d1 * d1 + d2 * d2)).sum() / n, f["q1"].sum() / n, y.sum() / n, np.abs(d1).sum() / n, over.sum() / n,
                      w.sum() / n, np.abs(f["q1"] - f["q2"]).sum() / n])
    return dict(out, td=y, stats=stats)


def torch_sac(inp, dtype, gamma=D.GAMMA, weight=True, perm=None):
    """The head as a torch user writes it, on the CPU in `dtype`, with autograd from q1 and q2 of L_critic = sum_i mean_b w ((Q1 - y)^2 +
    (Q2 - y)^2), y = r + gamma (1 - done) (min(Q1', Q2') - alpha logp') -> dict of float64 numpy.  perm: the rows in another order."""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
    la = t.pop("log_alpha")
    if perm is not None:
        t = {k: v[perm] for k, v in t.items()}
    q1, q2 = (t[k].clone().requires_grad_() for k in ("q1", "q2"))
    w = t["weight"] if weight else torch.ones_like(t["q1"])
    y = t["rew"] + gamma * (1.0 - t["done"].to(dtype)) * (torch.minimum(t["q1_next"], t["q2_next"]) - torch.exp(la) * t["logp_next"])
    ((w * (q1 - y) ** 2).mean(0).sum() + (w * (q2 - y) ** 2).mean(0).sum()).backward()
    gs = {k: torch.zeros((*q1.shape, 4), dtype=dtype) for k in ("g_q1", "g_q2")}
    gs["g_q1"][..., 0], gs["g_q2"][..., 0] = q1.grad, q2.grad
    gs["td"] = y
    if perm is not None:
        inv = torch.argsort(perm)
        gs = {k: v[inv] for k, v in gs.items()}
    with torch.no_grad():
        d1, d2 = q1 - y, q2 - y
        num = lambda x: float(x.double())                     # noqa: E731
        stats = np.array([float(q1.numel()), num((w * (d1 * d1 + d2 * d2)).mean()), num(q1.mean()), num(y.mean()), num(d1.abs().mean()),
                          num(t["done"].to(dtype).mean()), num(w.mean()), num((q1 - q2).abs().mean())])
    return dict({k: v.detach().double().numpy() for k, v in gs.items()}, stats=stats)


@functools.lru_cache(maxsize=None)
def sac_case(B, nA, weight=True, perms=8):
    """(inputs, float64 reference, float32 yardstick, the yardstick's own error on stats [8] over 9 row orders).  Read-only."""
    inp = sac_inputs(B, nA)
    ref, yard = ref_sac_head(inp, weight=weight), torch_sac(inp, torch.float32, weight=weight)
    return inp, ref, yard, Y.own_error(lambda order: torch_sac(inp, torch.float32, weight=weight, perm=order), ref, B, perms)[0]


head_id = T.head_id


def contract32(inp, gamma=D.GAMMA, weight=True):
    """The header's contract operation by operation in numpy float32 (each fmaf through float64: its product is exact there) -> the
    three tensors as float64 arrays: a float32 evaluation of the head equivalent to torch_sac's, in the kernel's association."""
    f = {k: v.numpy() for k, v in inp.items()}
    B, nA = f["q1"].shape
    w = f["weight"] if weight else np.ones((B, nA), np.float32)
    f64 = lambda x: x.astype(np.float64)                          # noqa: E731
    with np.errstate(all="ignore"):
        alpha = np.exp(f["log_alpha"]).astype(np.float32)[None]
        m = np.where((f["q1_next"] < f["q2_next"]) | (f["q1_next"] != f["q1_next"]), f["q1_next"], f["q2_next"])
        v = (f64(-alpha) * f64(f["logp_next"]) + f64(m)).astype(np.float32)
        qn = np.where(f["done"] != 0, np.float32(0.0), v)
        y = (np.float64(np.float32(gamma)) * f64(qn) + f64(f["rew"])).astype(np.float32)
    s2 = np.float32(2.0 / B)
    out = {k: np.zeros((B, nA, 4)) for k in ("g_q1", "g_q2")}
    out["g_q1"][..., 0], out["g_q2"][..., 0] = (w * (f["q1"] - y)) * s2, (w * (f["q2"] - y)) * s2
    return dict(out, td=y.astype(np.float64))


def head_spread(B, nA, weight=True, perms=8):
    """{tensor: (max ratio, mean ratio)}: how far the float32 yardstick's own error on the head's three tensors moves over equivalent
    float32 evaluations -- the contract's association (contract32) and torch_sac over yardstick_util.row_orders.  No kernel output enters."""
    inp, ref, yard, _ = sac_case(B, nA, weight)
    others = [contract32(inp, weight=weight)] + [torch_sac(inp, torch.float32, weight=weight, perm=o) for o in list(Y.row_orders(B, perms))[1:]]
    return U.spread(ref, yard, others, TD_NAMES)


def factors(B, nA, weight):
    """tensor -> (mean factor, max factor): the project's (2, 4), or what profiles/sac_float64.json records for the case from head_spread."""
    return Y.factor_of(Y.recorded(PROFILE, "factors").get(head_id(B, nA, weight), {}))


def check_sac(got, ref, yard, e_stats, what="", factor_of=None):
    """got: dict(g_q1, g_q2, td, stats) of float64 numpy from the kernel.  Prints every figure, then asserts."""
    bad = Y.check_tensors([(k, got[k], ref[k], yard[k], (factor_of or Y.factor_of({}))(k)) for k in TD_NAMES], what, unit="x")[1]
    bad += T.stats_out_of_bounds(got["stats"], ref["stats"], e_stats, what)
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------ the policy's seeds and gradients
def ref_policy_seed(q1, q2, w, B):
    """bsx_sac_policy_seed in numpy float32, bit for bit -> (g_pi1, g_pi2) [B, nA, 4].  w: float32 [B, nA] or None."""
    first = (q1 < q2) | (q1 != q1)
    seed = -((np.ones_like(q1) if w is None else w) * np.float32(1.0 / B))
    g1, g2 = np.zeros((*q1.shape, 4), np.float32), np.zeros((*q1.shape, 4), np.float32)
    g1[..., 0], g2[..., 0] = np.where(first, seed, np.float32(0.0)), np.where(first, np.float32(0.0), seed)
    return g1, g2


def policy_inputs(shape, seed=0):
    """sac_policy_grad's inputs at a shape, float32 CPU tensors: gx1, gx2 about 1 / B, normals z (column 3 = 0), logp, q1_pi, q2_pi (every
    16th pair equal), weights uniform in [0.5, 1.5], log_std about -1, log_alpha about log 0.2."""
    B, nA, Do, k, central = shape
    Dc = D.width(nA, Do, k, central)
    g = torch.Generator().manual_seed(8800 + seed + 7 * B + nA + Do + central)
    rnd = lambda *s: torch.randn(s, generator=g)                  # noqa: E731
    z = rnd(B, nA, 4)
    z[..., 3] = 0.0
    q1 = rnd(B, nA)
    q2 = q1 + 0.3 * rnd(B, nA)
    q2.view(-1)[::16] = q1.view(-1)[::16]
    return dict(gx1=rnd(B, nA, Dc) / B, gx2=rnd(B, nA, Dc) / B, z=z, logp=rnd(B, nA) - 1.0, q1_pi=q1, q2_pi=q2,
                weight=torch.rand((B, nA), generator=g) + 0.5, log_std=-1.0 + 0.3 * rnd(nA, 3), log_alpha=math.log(0.2) + 0.3 * rnd(nA))


def own_columns(gx, Do, central):
    """Agent i's own three action columns of row (b, i) -> [B, nA, 3] (numpy or torch)."""
    nA = gx.shape[1]
    cols = [(nA * Do + 3 * i if central else Do) for i in range(nA)]
    pick = [gx[:, i, c:c + 3] for i, c in enumerate(cols)]
    return np.stack(pick, 1) if isinstance(gx, np.ndarray) else torch.stack(pick, 1)


def ga32(gx1, gx2, Do, central):
    """g_a4 [B, nA, 4] in float32 numpy: the kernel's bits (one float32 add per column, column 3 +0)."""
    out = np.zeros((*gx1.shape[:2], 4), np.float32)
    out[..., :3] = own_columns(gx1, Do, central) + own_columns(gx2, Do, central)
    return out


def _policy(f, Do, central, te, weight, xp, B):
    """g_log_std [nA, 3], g_log_alpha [nA] and stats [8] from arrays or tensors f in their dtype (xp: numpy or torch)."""
    ga = own_columns(f["gx1"], Do, central) + own_columns(f["gx2"], Do, central)
    w = f["weight"] if weight else xp.ones_like(f["logp"])
    alpha = xp.exp(f["log_alpha"])
    ws = w * (1.0 / B)
    g_ls = (ga * (xp.exp(f["log_std"])[None] * f["z"][..., :3])).sum(0) - alpha[:, None] * ws.sum(0)[:, None]
    g_la = -(ws * (f["logp"] + te)).sum(0)
    first = (f["q1_pi"] < f["q2_pi"]) | (f["q1_pi"] != f["q1_pi"])
    m = xp.where(first, f["q1_pi"], f["q2_pi"])
    n = float(m.size if xp is np else m.numel())
    num = lambda x: float(x.sum()) / n if xp is np else float(x.double().mean())      # noqa: E731
    a_all = alpha[None] + 0.0 * m
    one = first.astype(np.float64) if xp is np else first.to(m.dtype)
    stats = np.array([n, num(w * (alpha[None] * f["logp"] - m)), num(m), num(f["logp"]), num(a_all), num(w), num(one), 0.0])
    return ga, g_ls, g_la, stats


def ref_policy_grad(inp, Do, central, te=TARGET_ENTROPY, weight=True):
    """sac_policy_grad's contract in float64 numpy -> dict(g_a4 [B, nA, 4], g_log_std, g_log_alpha, stats)."""
    f = {k: v.double().numpy() for k, v in inp.items()}
    B = f["logp"].shape[0]
    ga, g_ls, g_la, stats = _policy(f, Do, central, te, weight, np, B)
    return dict(g_a4=np.concatenate([ga, np.zeros((*ga.shape[:2], 1))], -1), g_log_std=g_ls, g_log_alpha=g_la, stats=stats)


def torch_policy_grad(inp, Do, central, te=TARGET_ENTROPY, weight=True, perm=None, dtype=torch.float32):
    """The same as a torch user writes it on the CPU in `dtype` (sums over the batch by torch) -> float64 numpy."""
    per_row = ("gx1", "gx2", "z", "logp", "q1_pi", "q2_pi", "weight")
    f = {k: (v.to(dtype)[perm] if perm is not None and k in per_row else v.to(dtype)) for k, v in inp.items()}
    _, g_ls, g_la, stats = _policy(f, Do, central, te, weight, torch, f["logp"].shape[0])
    return dict(g_log_std=g_ls.double().numpy(), g_log_alpha=g_la.double().numpy(), stats=stats)


@functools.lru_cache(maxsize=None)
def policy_case(shape, weight=True, perms=8):
    """(inputs, float64 reference, float32 yardstick, {stats, g_log_std, g_log_alpha: the yardstick's own error over 9 row orders}).
    Read-only."""
    _, _, Do, _, central = shape
    inp = policy_inputs(shape)
    ref, yard = ref_policy_grad(inp, Do, central, weight=weight), torch_policy_grad(inp, Do, central, weight=weight)
    own = Y.own_error(lambda o: torch_policy_grad(inp, Do, central, weight=weight, perm=o), ref, shape[0], perms, SUMS)
    return inp, ref, yard, dict(zip(SUMS, own))


SUMS = ("stats", "g_log_std", "g_log_alpha")


def sums_out_of_bounds(got, ref, own, name, what=""):
    """g_log_std and g_log_alpha are, per agent (and column), ONE sum over the batch rounded to float32 once -- a statistic, not a field of
    many elements: each is held the way yardstick_util holds a statistic, to scalar_bound of the float32 yardstick's own error on that
    element over nine row orders (never less than half a float32 spacing at its size: no float32 value can be expected closer).  Prints
    every figure -> the elements out of bounds."""
    bad = []
    for i in np.ndindex(ref.shape):
        tol, err = Y.scalar_bound(ref[i], own[i]), abs(got[i] - ref[i])
        print(f"{what} {name}{list(i)}: float64 {ref[i]:.9g}, kernel error {err:.3e}, yardstick's own (9 row orders) {own[i]:.3e}, bound {tol:.3e}")
        if not err <= tol:
            bad.append(f"{name}{list(i)}")
    return bad


def pi_stats_out_of_bounds(got, ref, e_stats, what=""):
    counts = [] if got[0] == ref[0] and got[7] == 0.0 else ["n"]
    return counts + Y.stats_out_of_bounds(got, ref, e_stats, PI_STAT_NAMES, what)


# ------------------------------------------------------------------------------------------------ the three losses under autograd
def losses(nets, targets, log_std, log_alpha, batch, w, z_next, z_pi, central, dtype, gamma=D.GAMMA, te=TARGET_ENTROPY, critics_pi=None,
           entropy=True, next_actor=None, through="min", ls_alpha=True):
    """(L_critic, L_pi, L_alpha, leaves, extras) on the CPU in `dtype`, as the issue writes them:
        L_critic = sum_i mean_b w ((Q1_i(x_cur) - y)^2 + (Q2_i(x_cur) - y)^2),  y = r + gamma (1 - done) (min(Q1'_i, Q2'_i)(x_next) -
                   alpha_i logp'), held fixed; x_next from a' = mu(o') + exp(log_std) z_next of the CURRENT actor
        L_pi     = sum_i mean_b w (alpha_i logp - min(Q1_i, Q2_i)(x_pi)),  a = mu(o) + exp(log_std) z_pi into slot i, z held fixed,
                   alpha held fixed; the critics: critics_pi (an update's stepped ones), nets[1:] if none
        L_alpha  = -sum_i log_alpha_i mean_b w (logp + target_entropy),  logp detached
    nets = (actor, critic, critic2), targets = (tc, tc2).  The misreadings: entropy=False (no entropy term in y), next_actor (a' from
    another network), through="first" (the actor through critic 1 alone), ls_alpha=False (logp detached in L_pi)."""
    to = lambda net: U._to(net, "cpu", dtype)                      # noqa: E731
    a, c1, c2 = (to(n) for n in nets)
    tc1, tc2 = (to(n) for n in targets)
    p1, p2 = (to(n) for n in critics_pi) if critics_pi is not None else (c1, c2)
    nxt = to(next_actor) if next_actor is not None else a
    obs, act, rew, obs_next = (t.detach().cpu().to(dtype) for t in batch[:4])
    notdone, w = 1.0 - batch[4].detach().cpu().to(dtype), w.detach().cpu().to(dtype)
    ls = log_std.detach().cpu().to(dtype).clone().requires_grad_()
    la = log_alpha.detach().cpu().to(dtype).clone().requires_grad_()
    zn, zp = z_next.to(dtype)[..., :3], z_pi.to(dtype)[..., :3]
    const = 1.5 * math.log(2.0 * math.pi)
    with torch.no_grad():
        alpha = torch.exp(la)
        lp_next = (-0.5 * zn * zn - ls).sum(-1) - const
        x_next = D.joined(obs_next, nxt(obs_next) + torch.exp(ls) * zn, central)
        q1n, q2n = tc1(x_next, squash=False)[..., 0], tc2(x_next, squash=False)[..., 0]
        y = rew + gamma * notdone * (torch.minimum(q1n, q2n) - (alpha * lp_next if entropy else 0.0))
    x_cur = D.joined(obs, act, central)
    q1, q2 = c1(x_cur, squash=False)[..., 0], c2(x_cur, squash=False)[..., 0]
    l_critic = (w * (q1 - y) ** 2).mean(0).sum() + (w * (q2 - y) ** 2).mean(0).sum()
    logp = (-0.5 * zp * zp - ls).sum(-1) - const
    act_pi = a(obs) + torch.exp(ls) * zp
    x_pi = D.joined_pi(obs, act, act_pi, central)
    q1p, q2p = p1(x_pi, squash=False)[..., 0], p2(x_pi, squash=False)[..., 0]
    mq = torch.minimum(q1p, q2p) if through == "min" else q1p
    l_pi = (w * (alpha * (logp if ls_alpha else logp.detach()) - mq)).mean(0).sum()
    l_alpha = -(la * (w * (logp.detach() + te)).mean(0)).sum()
    extras = dict(q1=q1, q2=q2, q1_next=q1n, q2_next=q2n, logp_next=lp_next, y=y, logp=logp, q1_pi=q1p, q2_pi=q2p, x_pi=x_pi, act_pi=act_pi)
    return l_critic, l_pi, l_alpha, dict(actor=a, critic=c1, critic2=c2, log_std=ls, log_alpha=la), extras


def sac_grads(*args, **kw):
    """losses' gradients -> dict(gc1, gc2, ga: {tensor: float64 array}; g_ls [nA, 3], g_la [nA]; extras: float64-or-dtype tensors)."""
    l_c, l_pi, l_a, leaf, ex = losses(*args, **kw)
    num = lambda gs: {p: t.double().numpy() for p, t in zip(PARAMS, gs)}            # noqa: E731
    g = torch.autograd.grad(l_c, [getattr(n, p) for n in (leaf["critic"], leaf["critic2"]) for p in PARAMS])
    gp = torch.autograd.grad(l_pi, [getattr(leaf["actor"], p) for p in PARAMS] + [leaf["log_std"]])
    g_la, = torch.autograd.grad(l_a, [leaf["log_alpha"]])
    return dict(gc1=num(g[:10]), gc2=num(g[10:]), ga=num(gp[:10]), g_ls=gp[10].double().numpy(), g_la=g_la.double().numpy(),
                extras={k: v.detach() for k, v in ex.items()})


# ------------------------------------------------------------------------------------------------ one update by hand
STATE = T.STATE + ("stats_pi", "log_std", "log_alpha", "step_alpha")


def snapshot(x):
    """td3_util.snapshot plus what SAC adds: the policy's statistics, log_std, log_alpha, their moments and the temperature's step count."""
    out = T.snapshot(x)
    bits = lambda t: t.detach().view(torch.int32 if t.dtype == torch.float32 else torch.int64).clone()     # noqa: E731
    out.update(stats_pi=bits(x.stats_pi), log_std=bits(x.log_std), log_alpha=bits(x.log_alpha), step_alpha=x.step_alpha.clone())
    out["adam_log_std.m"], out["adam_log_std.v"] = bits(x.adam_log_std.m), bits(x.adam_log_std.v)
    if x.adam_alpha is not None:
        out["adam_alpha.m"], out["adam_alpha.v"] = bits(x.adam_alpha.m), bits(x.adam_alpha.v)
    return out


blobs_are_packs = T.blobs_are_packs


class Hand(D.Hand):
    """What a SACLearner holds, under the same names, and its update written out with the public primitives alone."""

    def __init__(self, buffer, actor, critic, critic2, central, log_std=None, alpha=0.2, lr_alpha=3e-4, target_entropy=TARGET_ENTROPY, seed=0,
                 **kw):
        from deep_rl_battlespace_amd import learner as L
        super().__init__(buffer, actor, critic, central, **kw)
        dev, nA = actor.w1.device, actor.n_actors
        self.critic2, self.target_critic2 = critic2, copy.deepcopy(critic2)
        self.target_critic2.__dict__.pop("_bsx_mlp_buffers", None)
        self._blob_c2, self._blob_tc2 = critic2.pack(), self.target_critic2.pack()
        self.adam_critic2 = L.AdamState(critic2)
        self.log_std = log_std if log_std is not None else torch.full((nA, 3), math.log(0.2), dtype=torch.float32, device=dev)
        self.adam_log_std = L.AdamState(self.log_std)
        self.log_alpha = torch.full((nA,), math.log(alpha), dtype=torch.float32, device=dev)
        self.adam_alpha = L.AdamState(self.log_alpha) if lr_alpha is not None else None
        self.hyper_alpha = L.adam_hyper(lr_alpha, kw.get("betas", (0.9, 0.999)), kw.get("eps", 1e-8), None, dev) if lr_alpha is not None else None
        self.step_alpha = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stats_pi = torch.zeros((self.updates, 8), dtype=torch.float64, device=dev)
        self.target_entropy, self.seed = target_entropy, seed
        self._noise_draws = torch.zeros(1, dtype=torch.int64, device=dev)
        self.prioritized = hasattr(buffer, "tree")

    def update(self):
        for u in range(self.updates):
            s = self.buffer.sample()
            self.step(s[0].transpose(0, 1), s[2].transpose(0, 1), s[3], s[4].transpose(0, 1), s[6], u,
                      weight=self.buffer.weights if self.prioritized else None)
        return self.stats

    def step(self, obs, act, rew, obs_next, done, u, weight=None, z_next=None, z_pi=None):
        """The ten steps on a batch -> dict(row_c, row_c2, row_a: copies of mlp_grad's cached rows; g_log_std, g_log_alpha: copies).
        z_next, z_pi: the two draws' normals, injected (the sequence word stays)."""
        from deep_rl_battlespace_amd import _lib, learner as L
        lib, c = _lib.load(), self.central
        obs, act, obs_next = obs.contiguous(), act.contiguous(), obs_next.contiguous()
        (B, nA, Do), k, dev = obs.shape, act.shape[2], obs.device
        stream = torch.cuda.current_stream(dev).cuda_stream

        def forward(blob, x, raw=False):
            y4 = torch.empty((B, nA, 4), device=dev)
            r = torch.empty((B, nA), device=dev) if raw else None
            _lib.check(lib.bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y4.data_ptr(), r.data_ptr() if raw else None, B, nA, x.shape[2], stream),
                       "bsx_mlp_forward")
            return r if raw else y4

        def draw(y4, x, own_only, z):
            if z is not None:
                return L.sac_sample_actions(y4, self.log_std, x, Do, k, seed=self.seed, z=z, central=c, own_only=own_only)
            out = L.sac_sample_actions(y4, self.log_std, x, Do, k, seed=self.seed, seq_base=self._noise_draws, central=c, own_only=own_only)
            self._noise_draws.add_(1)
            return out
        x_cur, x_next, x_pi = L.ddpg_inputs(obs, obs_next, act, central=c)
        _, logp_next, _ = draw(forward(self._blob_a, obs_next), x_next, False, z_next)
        q1_next, q2_next = forward(self._blob_tc, x_next, True), forward(self._blob_tc2, x_next, True)
        q1, q2 = forward(self._blob_c, x_cur, True), forward(self._blob_c2, x_cur, True)
        head = L.sac_head(q1, q2, q1_next, q2_next, logp_next, rew, done, self.log_alpha, self.gamma, weight=weight)
        self.stats[u].copy_(head.stats)
        self.td = head.td
        if self.prioritized:
            self.buffer.update_priorities(q1, head.td)
        row_c = L.mlp_grad(self.critic, self._blob_c, x_cur, head.g_q1[..., :1].contiguous(), squash=False, input_grad=False)[0].clone()
        row_c2 = L.mlp_grad(self.critic2, self._blob_c2, x_cur, head.g_q2[..., :1].contiguous(), squash=False, input_grad=False)[0].clone()
        L.mlp_adam_step([self.critic, self.critic2], [row_c, row_c2], [self.adam_critic, self.adam_critic2], [self._blob_c, self._blob_c2],
                        self.hyper_critic, self.step_critic, targets=[self.target_critic, self.target_critic2],
                        target_blobs=[self._blob_tc, self._blob_tc2], stats=self.step_stats_critic[u])
        _, logp, z = draw(forward(self._blob_a, obs), x_pi, True, z_pi)
        q1_pi, q2_pi = forward(self._blob_c, x_pi, True), forward(self._blob_c2, x_pi, True)
        s1, s2 = L.sac_policy_seed(q1_pi, q2_pi, weight=weight)
        _, gx1 = L.mlp_grad(self.critic, self._blob_c, x_pi, s1[..., :1].contiguous(), squash=False, input_grad=True)
        _, gx2 = L.mlp_grad(self.critic2, self._blob_c2, x_pi, s2[..., :1].contiguous(), squash=False, input_grad=True)
        pg = L.sac_policy_grad(gx1, gx2, z, logp, q1_pi, q2_pi, self.log_std, self.log_alpha, Do, k, target_entropy=self.target_entropy,
                               weight=weight, central=c, alpha_state=self.adam_alpha, hyper=self.hyper_alpha,
                               step=self.step_alpha if self.adam_alpha is not None else None)
        self.stats_pi[u].copy_(pg.stats)
        row_a = L.mlp_grad(self.actor, self._blob_a, obs, pg.g_a4[..., :k].contiguous(), squash=True, input_grad=False)[0].clone()
        L.mlp_adam_step([self.actor], [row_a], [self.adam_actor], [self._blob_a], self.hyper_actor, self.step_actor, log_std=self.log_std,
                        g_log_std=pg.g_log_std, log_std_state=self.adam_log_std, stats=self.step_stats_actor[u])
        return dict(row_c=row_c, row_c2=row_c2, row_a=row_a, g_log_std=pg.g_log_std.clone(), g_log_alpha=pg.g_log_alpha.clone())


# ------------------------------------------------------------------------------------------------ a whole update against float64
ALPHA_LR = 3e-4


def _actor_step(actor, ga, log_std, g_ls, kw, dtype):
    """The actor's step with log_std in the same call (one clip norm over both, no targets) -> td3_util._joint_step64's dict plus
    log_std, m_ls, v_ls.  float64: adam_mlp_util.reference_step; float32: clip_grad_norm_ and torch.optim.Adam over the eleven tensors."""
    hp = AU.hyper32(kw["lr_actor"], *kw["betas"], kw["eps"], kw["max_grad_norm"] or 0.0)
    if dtype == torch.float64:
        P0 = AU.net_arrays(actor) + [log_std.detach().cpu().numpy()]
        Z = [np.zeros(x.shape) for x in P0]
        P, M_, V, _, _, norm, coef = AM.reference_step(P0, [ga[p] for p in PARAMS] + [g_ls], Z, Z, [None] * 11, 0, hp, 0.0)
        return dict(p=P[:10], m=M_[:10], v=V[:10], ls=dict(p=[P[10]], m=[M_[10]], v=[V[10]]), norm=norm, coef=coef)
    ps = [getattr(actor, p).detach().clone().float().requires_grad_() for p in PARAMS] + [log_std.detach().clone().float().requires_grad_()]
    for p, g in zip(ps, [ga[name] for name in PARAMS] + [g_ls]):
        p.grad = torch.from_numpy(np.ascontiguousarray(g)).float()
    if hp["max_grad_norm"] > 0.0:
        torch.nn.utils.clip_grad_norm_(ps, hp["max_grad_norm"])
    opt = torch.optim.Adam(ps, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    opt.step()
    f = lambda xs: [x.detach().numpy() for x in xs]               # noqa: E731
    m, v = f([opt.state[p]["exp_avg"] for p in ps]), f([opt.state[p]["exp_avg_sq"] for p in ps])
    return dict(p=f(ps[:10]), m=m[:10], v=v[:10], ls=dict(p=f(ps[10:]), m=m[10:], v=v[10:]))


def _alpha_step(log_alpha, g_la, kw, dtype):
    """log_alpha's Adam step without clipping -> dict(p, m, v: one-element lists)."""
    hp = AU.hyper32(ALPHA_LR, *kw["betas"], kw["eps"], 0.0)
    if dtype == torch.float64:
        P, M_, V, *_ = AU.reference_step([log_alpha.detach().cpu().numpy()], [g_la], [np.zeros(g_la.shape)], [np.zeros(g_la.shape)], 0, hp)
        return dict(p=P, m=M_, v=V)
    p = log_alpha.detach().clone().float().requires_grad_()
    p.grad = torch.from_numpy(np.ascontiguousarray(g_la)).float()
    opt = torch.optim.Adam([p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    opt.step()
    return dict(p=[p.detach().numpy()], m=[opt.state[p]["exp_avg"].numpy()], v=[opt.state[p]["exp_avg_sq"].numpy()])


def update_reference(nets, targets, log_std, log_alpha, batch, w, z_next, z_pi, central, dtype, kw=None, perm=None, **variant):
    """One whole SAC update on the CPU in `dtype` -> dict(gc1, gc2, ga, g_ls, g_la; critic, critic2 (the joint step with both Polyak
    targets), actor (with ls: log_std's part), alpha: the steps; head, pi: the inputs of ref_sac_head / ref_policy_grad's statistics)."""
    kw = kw or D.STEP_KW
    if perm is not None:
        batch, w, z_next, z_pi = tuple(t[perm] for t in batch), w[perm], z_next[perm], z_pi[perm]
    args = (nets, targets, log_std, log_alpha, batch, w, z_next, z_pi, central, dtype, kw["gamma"])
    first = sac_grads(*args, **variant)
    step = T._joint_step64 if dtype == torch.float64 else T._joint_step32
    s1, s2 = step(nets[1:], [first["gc1"], first["gc2"]], targets, kw["lr_critic"], kw)
    second = sac_grads(*args, critics_pi=(s1["net"], s2["net"]), **variant)
    ex1, ex2 = first["extras"], second["extras"]
    head = dict(q1=ex1["q1"], q2=ex1["q2"], q1_next=ex1["q1_next"], q2_next=ex1["q2_next"], logp_next=ex1["logp_next"], rew=batch[2].to(dtype),
                done=batch[4].to(torch.uint8), weight=w.to(dtype), log_alpha=log_alpha.to(dtype))
    pi = dict(logp=ex2["logp"], q1_pi=ex2["q1_pi"], q2_pi=ex2["q2_pi"], weight=w.to(dtype), log_alpha=log_alpha.to(dtype))
    return dict(gc1=first["gc1"], gc2=first["gc2"], ga=second["ga"], g_ls=second["g_ls"], g_la=second["g_la"], critic=s1, critic2=s2,
                actor=_actor_step(nets[0], second["ga"], log_std, second["g_ls"], kw, dtype), alpha=_alpha_step(log_alpha, second["g_la"], kw, dtype),
                head=head, pi=pi, x_pi=ex2["x_pi"].contiguous())


def pi_stats(pi, dtype=torch.float64):
    """SAC_PI_STATS of update_reference's `pi` in `dtype` -> float64 [8]."""
    f = {k: v.to(dtype) for k, v in pi.items()}
    alpha = torch.exp(f["log_alpha"])[None]
    first = f["q1_pi"] < f["q2_pi"]
    m = torch.where(first, f["q1_pi"], f["q2_pi"])
    num = lambda x: float(x.double().mean()) if dtype == torch.float32 else float(x.mean())      # noqa: E731
    return np.array([float(m.numel()), num(f["weight"] * (alpha * f["logp"] - m)), num(m), num(f["logp"]), num(alpha + 0.0 * m), num(f["weight"]),
                     num(first.to(dtype)), 0.0])


def _kinks(ref, x_pi):
    """Rows within KINK of a kink of either stepped critic at x_pi, or with |q1_pi - q2_pi| within KINK of 0 (float64)."""
    near = U.near_kink((ref["critic"]["net"], x_pi), (ref["critic2"]["net"], x_pi))
    return near | ((ref["pi"]["q1_pi"] - ref["pi"]["q2_pi"]).abs() <= U.KINK)


def try_seed(shape, seed):
    """stepped_case's construction at a seed -> (a namespace, or None where the filter does not close within MAX_ROUNDS; share; rounds)."""
    B, nA, Do, k, central = shape
    actor, critic, rows, idx, *_ = D.learner_case(shape, seed)
    critic2 = T.critic2_of(shape, seed)
    g = torch.Generator().manual_seed(9850 + seed)
    nets = (actor, critic, critic2)
    targets = tuple(D.perturbed(n, g) for n in nets[1:])
    batch = tuple(r[idx] for r in rows)
    z_next, z_pi = torch.randn((B, nA, 4), generator=g), torch.randn((B, nA, 4), generator=g)
    z_next[..., 3], z_pi[..., 3] = 0.0, 0.0
    log_std = -1.0 + 0.3 * torch.randn((nA, 3), generator=g)
    log_alpha = math.log(0.2) + 0.3 * torch.randn((nA,), generator=g)
    w = torch.randn((B, nA), generator=g)
    x_cur = D.joined(batch[0].double(), batch[1].double(), central).contiguous()
    w[U.near_kink((actor, batch[0]), (critic, x_cur), (critic2, x_cur))] = 0.0
    rounds = 0
    while True:
        ref = update_reference(nets, targets, log_std, log_alpha, batch, w, z_next, z_pi, central, torch.float64)
        near = _kinks(ref, ref["x_pi"]) & (w != 0)
        if not near.any():
            break
        rounds += 1
        if rounds > D.MAX_ROUNDS:
            return None, float((w == 0).double().mean()), rounds
        w[near] = 0.0
    case = types.SimpleNamespace(seed=seed, nets=nets, targets=targets, rows=rows, idx=idx, batch=batch, z_next=z_next, z_pi=z_pi, log_std=log_std,
                                 log_alpha=log_alpha, w=w, rounds=rounds, share=float((w == 0).double().mean()), ref=ref)
    return case, case.share, rounds


@functools.lru_cache(maxsize=None)
def stepped_case(shape, seed=None):
    """One SAC update (ddpg_util.STEP_KW, the temperature's rate ALPHA_LR) from ddpg_util.learner_case's actor, critic, ring rows and idx,
    critic2_of's second critic, two target critics that are NOT the critics (each parameter plus 0.05 randn), injected normals for both
    draws, random log_std (about -1) and log_alpha (about log 0.2), on the CPU.  w: standard normal row weights, 0 where, in float64, any
    of these lies within actor_grad_util.KINK of 0: a pre-ReLU value of either critic at x_cur, of the actor at obs, of either STEPPED
    critic at x_pi, or |q1_pi - q2_pi| -- iterated to a fixed point (at most ddpg_util.MAX_ROUNDS zeroing rounds).  ref, yard:
    update_reference in float64 and float32; the statistics rows and the yardstick's own error over 9 row orders.  Read-only."""
    seed = STEP_SEEDS.get(tuple(shape), 0) if seed is None else seed
    c, share, rounds = try_seed(shape, seed)
    assert c is not None, (shape, seed, share, rounds)
    central, B = shape[4], shape[0]
    run = lambda order=None: update_reference(c.nets, c.targets, c.log_std, c.log_alpha, c.batch, c.w, c.z_next, c.z_pi, central,      # noqa: E731
                                              torch.float32, perm=order)
    c.yard = run()
    c.stats, c.stats_pi = ref_sac_head(c.ref["head"])["stats"], pi_stats(c.ref["pi"])
    c.e_stats = Y.own_error(lambda order: torch_sac(c.yard["head"], torch.float32, perm=order), dict(stats=c.stats), B)[0]
    perm_pi = lambda order: dict(stats=pi_stats({k: (v[order] if order is not None and v.dim() == 2 else v) for k, v in c.yard["pi"].items()},      # noqa: E731
                                                torch.float32))
    c.e_stats_pi = Y.own_error(perm_pi, dict(stats=c.stats_pi), B)[0]
    return c


SMALL = ("g_ls", "g_la", "log_std.p", "log_std.m", "log_std.v", "log_alpha.p", "log_alpha.m", "log_alpha.v")


def small(r):
    """The quantities of an update_reference result with one value per agent (and column) -> {name of SMALL: array}: log_std's and
    log_alpha's gradients and what their steps leave."""
    out = dict(g_ls=r["g_ls"], g_la=r["g_la"])
    for name, step in (("log_std", r["actor"]["ls"]), ("log_alpha", r["alpha"])):
        out.update({f"{name}.{k}": np.asarray(step[k][0], np.float64) for k in ("p", "m", "v")})
    return out


def stepped_spread(shape, perms=8):
    """{name of SMALL: (max ratio, mean ratio)}: how far the float32 yardstick's own error on log_std's and log_alpha's gradients and
    steps of stepped_case moves when the batch's rows are summed in another order (actor_grad_util.spread over
    yardstick_util.row_orders).  With one agent log_std's are three numbers and log_alpha's one: their error is a few draws of a
    rounding.  No kernel output enters."""
    c = stepped_case(shape)
    others = [small(update_reference(c.nets, c.targets, c.log_std, c.log_alpha, c.batch, c.w, c.z_next, c.z_pi, shape[4], torch.float32, perm=order))
              for order in list(Y.row_orders(shape[0], perms))[1:]]
    return U.spread(small(c.ref), small(c.yard), others, SMALL)


def stepped_factor_of(shape):
    """name of SMALL -> (fm, fx) for stepped_case: the exception profiles/sac_float64.json records from stepped_spread, else (2, 4)."""
    return Y.factor_of(Y.recorded(PROFILE, "stepped", "factors").get(D.shape_id(shape), {}))


def wrong_variants(case, central):
    """{name: (|wrong - right| mean per tensor, the yardstick's mean error per tensor)} in float64: the four misreadings of the issue."""
    c = case
    g = torch.Generator().manual_seed(77)
    f = lambda **v: update_reference(c.nets, c.targets, c.log_std, c.log_alpha, c.batch, c.w, c.z_next, c.z_pi, central, torch.float64, **v)     # noqa: E731
    dist = lambda a, b: {p: float(np.abs(a[p] - b[p]).mean()) for p in D.SHARP}       # noqa: E731
    out = {}
    for name, variant, which in (("the entropy term left out of y", dict(entropy=False), "gc1"),
                                 ("next actions from a perturbed copy of the actor", dict(next_actor=D.perturbed(c.nets[0], g)), "gc1"),
                                 ("the actor through critic 1 alone", dict(through="first"), "ga")):
        out[name] = (dist(f(**variant)[which], c.ref[which]), dist(c.yard[which], c.ref[which]))
    wrong = f(ls_alpha=False)["g_ls"]
    out["g_log_std without its -alpha term"] = ({"log_std": float(np.abs(wrong - c.ref["g_ls"]).mean())},
                                                {"log_std": float(np.abs(c.yard["g_ls"] - c.ref["g_ls"]).mean())})
    return out


# ------------------------------------------------------------------------------------------------ the torch composition, the bandit
BANDIT = dict(D.BANDIT, k=3, alpha=0.02)


def torch_update(nets, targets, log_std, log_alpha, opt_a, opt_c, batch, central, gen, gamma=D.GAMMA, tau=0.01):
    """One SAC update with a fixed temperature the way a torch user writes it: autograd through StackedActor, one Adam over both critics
    with the Polyak lines of both targets, one Adam over the actor and log_std."""
    actor, c1, c2 = nets
    tc1, tc2 = targets
    obs, act, rew, obs_next, done = batch
    alpha, const = torch.exp(log_alpha), 1.5 * math.log(2.0 * math.pi)
    draw = lambda: torch.randn((*obs.shape[:2], 3), generator=gen, device=obs.device, dtype=obs.dtype)     # noqa: E731
    with torch.no_grad():
        z = draw()
        x_next = D.joined(obs_next, actor(obs_next) + torch.exp(log_std) * z, central)
        lp = (-0.5 * z * z - log_std).sum(-1) - const
        y = rew + gamma * (1.0 - done.to(rew.dtype)) * (torch.minimum(tc1(x_next, squash=False)[..., 0], tc2(x_next, squash=False)[..., 0]) - alpha * lp)
    x_cur = D.joined(obs, act, central)
    opt_c.zero_grad(set_to_none=True)
    (((c1(x_cur, squash=False)[..., 0] - y) ** 2).mean(0).sum() + ((c2(x_cur, squash=False)[..., 0] - y) ** 2).mean(0).sum()).backward()
    opt_c.step()
    with torch.no_grad():
        for t, n in zip(targets, nets[1:]):
            ts, ns = list(t.parameters()), list(n.parameters())
            torch._foreach_mul_(ts, 1.0 - tau)
            torch._foreach_add_(ts, ns, alpha=tau)
    z = draw()
    logp = (-0.5 * z * z - log_std).sum(-1) - const
    x_pi = D.joined_pi(obs, act, actor(obs) + torch.exp(log_std) * z, central)
    opt_a.zero_grad(set_to_none=True)
    (alpha * logp - torch.minimum(c1(x_pi, squash=False)[..., 0], c2(x_pi, squash=False)[..., 0])).mean(0).sum().backward()
    opt_a.step()


def bandit_rows(seed=0):
    """ddpg_util.bandit_rows at k = 3 (bandit_reward is generic in k)."""
    b = BANDIT
    g = torch.Generator().manual_seed(9900 + seed)
    uni = lambda *s: torch.rand(s, generator=g) * 2 - 1       # noqa: E731
    obs, act = uni(b["rows"], b["nA"], b["Do"]), uni(b["rows"], b["nA"], b["k"])
    rows = (obs, act, D.bandit_reward(obs, act), uni(b["rows"], b["nA"], b["Do"]), torch.ones((b["rows"], b["nA"]), dtype=torch.bool))
    return rows, uni(b["held_out"], b["nA"], b["Do"])


def bandit_nets(seed=0):
    """(actor, critic, critic2) on the CPU, freshly initialised (own critics: 8 -> 1)."""
    b = BANDIT
    torch.manual_seed(9950 + seed)
    return R._new(b["nA"], b["Do"], b["k"]), R._new(b["nA"], b["Do"] + b["k"], 1), R._new(b["nA"], b["Do"] + b["k"], 1)


def bandit_torch_run(N, seed=0):
    """(initial reward, reward after N updates) of the torch composition of SAC (fixed alpha) on the bandit, on the CPU; the reward is
    that of the policy's mean action."""
    b = BANDIT
    rows, held = bandit_rows(seed)
    nets = bandit_nets(seed)
    targets = tuple(copy.deepcopy(n) for n in nets[1:])
    log_std = torch.full((b["nA"], 3), math.log(0.2), requires_grad=True)
    log_alpha = torch.full((b["nA"],), math.log(b["alpha"]))
    oa = torch.optim.Adam(list(nets[0].parameters()) + [log_std], lr=b["lr"])
    oc = torch.optim.Adam(list(nets[1].parameters()) + list(nets[2].parameters()), lr=b["lr"])
    g = torch.Generator().manual_seed(9990 + seed)
    with torch.no_grad():
        r0 = float(D.bandit_reward(held, nets[0](held)).mean())
    for _ in range(N):
        idx = torch.randint(0, b["rows"], (b["B"],), generator=g)
        torch_update(nets, targets, log_std, log_alpha, oa, oc, tuple(r[idx] for r in rows), False, g, tau=b["tau"])
    with torch.no_grad():
        return r0, float(D.bandit_reward(held, nets[0](held)).mean())
