"""What the tests of the PPO loss head (learner.ppo_head, csrc/bsx_ppo_head.hip) share:

  reference        the contract of include/battlespace_hip.h (bsx_ppo_head) restated in float64 numpy: g_pi, g_v, g_log_std, stats
  torch_loss       the same loss written the way a user would (log_softmax / gather / clamp / torch.minimum / torch.maximum, as
                   tests/actor_grad_util.py::_ppo words it) with autograd from y, v (and log_std): in float64 the check of the
                   restatement, in float32 the yardstick -- what float32 itself loses on these inputs
  build            inputs: a behaviour policy y_old and a learner policy y a `step` away in pre-tanh space; categorical rec = y_old /
                   temperature + Gumbel noise, Gaussian rec = y_old + exp(log_std) z; logp_old from y_old; adv, v_old, v, ret normals;
                   mask Bernoulli 0.8; everything rounded to float32 ONCE (every path starts from the same float32 values)
  kink_filter      clears mask where, in float64, the ratio is within KINK of 1 +- clip, |v - v_old| within KINK of vclip, or the two
                   value branches within KINK of each other while clamped: there float32 and float64 may take different branches of the
                   loss and a row's whole gradient moves, for the reason actor_grad_util.py states for ReLU kinks
  case             the smallest step of LADDER for which 5 % .. 60 % of the kept rows have a ratio outside [1 - clip, 1 + clip] -- chosen
                   on the float64 reference alone --, its filtered inputs, the float64 reference and the float32 yardstick, cached
  check            yardstick_util's bounds: per gradient tensor (2 x mean, 4 x max) of the yardstick's error (except where
                   profiles/ppo_head_float64.json records a wider factor and why); stats and g_log_std within its scalar_bound of
                   own_errors, the yardstick's own error over 9 row orders

Nothing here imports the native library."""
import functools
import math
import os

import numpy as np
import torch

import yardstick_util as Y

KINK = 1e-4
LADDER = (0.03, 0.06, 0.12, 0.25, 0.5, 1.0)
CLIP, VCLIP, TAU, C_V, C_E = 0.2, 0.2, 0.7, 0.5, 0.01
FILTER_CAP = 0.01                       # the filter may remove at most 1 % of the masked rows
# (R, n) of the float64 test.  Up to n = 4 a workgroup's 256 threads are all at work (S = 256 or 252 of them) and the per-agent log_std
# reduction runs on 8 threads per column; the wide teams take its other forms and other merge shapes: n = 5 (A = 10: S = 250, 8 parts),
# n = 11 (A = 22: S = 242, 66 columns, 3 parts), n = 13 (A = 26: S = 234, 78 columns, 3 parts), n = 16 (A = 32: 96 columns, 2 parts, partial
# rows of 104 doubles)
SHAPES = ((1000, 1), (257, 3), (512, 4), (257, 5), (130, 11), (97, 13), (200, 16))
RAGGED_SHAPES = {1: SHAPES[0], 3: SHAPES[1], 11: SHAPES[4], 16: SHAPES[6]}       # n -> the shape the ragged test cuts its rows off
LARGE = (262209, 1)                     # 2 049 tiles of 256 elements (the last one ragged): beyond 2 048 a workgroup of the head pass takes two tiles
LARGE_STEP = dict(categorical=0.25, gaussian=0.06)               # the step the ladder ends on at (1000, 1): the ladder itself is not run at this size
KINDS = ("categorical", "gaussian")
LOG_2PI = math.log(2.0 * math.pi)
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ppo_head_float64.json")
STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl")      # stats[1..5]; stats[0] = N and stats[6] are counts


def build(kind, rows, n, step, seed=0):
    """{name: float32 / uint8 CPU tensor}: y, v, rec, logp_old, adv, ret, mask, v_old[, log_std]."""
    A = 2 * n
    g = torch.Generator().manual_seed(7000 + seed)
    rnd = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)    # noqa: E731
    pre = rnd(rows, A, 4)
    d_pre, u, z = rnd(rows, A, 4), torch.rand((rows, A, 4), generator=g, dtype=torch.float64), rnd(rows, A, 4)
    adv, v_old, dv, ret = rnd(rows, A), rnd(rows, A), rnd(rows, A), rnd(rows, A)
    mask = (torch.rand((rows, A), generator=g) < 0.8).to(torch.uint8)
    log_std = torch.rand((A, 3), generator=g, dtype=torch.float64) - 1.0          # in [-1, 0)
    y_old = torch.tanh(pre).float()
    y = torch.tanh(pre + step * d_pre).float()
    out = dict(adv=adv.float(), v_old=v_old.float(), v=(v_old + 0.3 * dv).float(), ret=ret.float(), mask=mask)
    if kind == "categorical":
        rec = (y_old.double() / TAU - torch.log(-torch.log(u))).float()
        lp = torch.log_softmax(y_old.double() / TAU, -1)
        out.update(y=y, rec=rec, logp_old=lp.gather(-1, rec.argmax(-1, keepdim=True)).squeeze(-1).float())
    else:
        y_old[..., 3], y[..., 3] = 0.0, 0.0
        ls = log_std.float()
        rec = torch.zeros((rows, A, 4))
        rec[..., :3] = (y_old[..., :3].double() + torch.exp(ls.double()) * z[..., :3]).float()
        zz = (rec[..., :3].double() - y_old[..., :3].double()) * torch.exp(-ls.double())
        out.update(y=y, rec=rec, log_std=ls, logp_old=((-0.5 * zz * zz - ls.double()).sum(-1) - 1.5 * LOG_2PI).float())
    return out


def head(inp, rows):
    """The first `rows` rows of an input set (views)."""
    return {k: (v if k == "log_std" else v[:rows]) for k, v in inp.items()}


def reference(inp, kind, vold=True, clip=CLIP, vclip=VCLIP, tau=TAU, c_v=C_V, c_e=C_E):
    """The contract in float64 numpy -> dict(g_pi [R, A, 4], g_v [R, A, 4], g_log_std [A, 3] or None, stats [8], ratio, clipped, vdiff,
    vgap [R, A]): vdiff = |v - v_old|, vgap = |(vc - ret)^2 - (v - ret)^2| (the value branches' distance)."""
    f = {k: v.double().numpy() for k, v in inp.items()}
    on = f["mask"] != 0
    y, rec, adv = f["y"], f["rec"], f["adv"]
    rows, A = adv.shape
    N = float(on.sum())
    dl, dh = np.zeros((rows, A, 4)), np.zeros((rows, A, 4))
    with np.errstate(all="ignore"):
        if kind == "categorical":
            s = y / tau
            s = s - s.max(-1, keepdims=True)
            lp = s - np.log(np.exp(s).sum(-1, keepdims=True))
            p = np.exp(lp)
            star = np.where(np.isnan(rec).any(-1), 0, np.argmax(np.nan_to_num(rec, nan=-np.inf), -1))      # the first maximum
            logp = np.take_along_axis(lp, star[..., None], -1)[..., 0]
            H = -(p * lp).sum(-1)
            dl = ((np.arange(4) == star[..., None]) - p) / tau
            dh = -p * (lp + H[..., None]) / tau
            z2 = None
        else:
            ls = f["log_std"]
            z = (rec[..., :3] - y[..., :3]) * np.exp(-ls)
            z2 = z * z
            logp = (-0.5 * z2 - ls).sum(-1) - 1.5 * LOG_2PI
            H = np.broadcast_to(ls.sum(-1) + 1.5 * (1.0 + LOG_2PI), (rows, A))
            dl[..., :3] = z * np.exp(-ls)
        lr = logp - f["logp_old"]
        ratio = np.exp(lr)
        surr = np.minimum(ratio * adv, np.clip(ratio, 1 - clip, 1 + clip) * adv)
        clipped = ((adv > 0) & (ratio > 1 + clip)) | ((adv < 0) & (ratio < 1 - clip))
        ds = np.where(clipped, 0.0, ratio * adv)
        d = f["v"] - f["ret"]
        lv, dlv = 0.5 * d * d, d.copy()
        vdiff = np.abs(f["v"] - f["v_old"])
        vc = f["v_old"] + np.clip(f["v"] - f["v_old"], -vclip, vclip)
        vgap = np.abs((vc - f["ret"]) ** 2 - d * d)
        if vold:
            worse = (vdiff > vclip) & ((vc - f["ret"]) ** 2 > d * d)
            lv = np.where(worse, 0.5 * (vc - f["ret"]) ** 2, lv)
            dlv = np.where(worse, 0.0, dlv)
        loss = -surr + c_v * lv - c_e * H
        g_pi = np.where(on[..., None], (-ds[..., None] * dl - c_e * dh) / max(N, 1.0), 0.0)
        g_v = np.zeros((rows, A, 4))
        g_v[..., 0] = np.where(on, c_v * dlv / max(N, 1.0), 0.0)
        g_ls = None
        if kind == "gaussian":
            g_ls = np.where(on[..., None], -ds[..., None] * (z2 - 1.0) - c_e, 0.0).sum(0) / max(N, 1.0)
        mean = lambda x: float(np.where(on, x, 0.0).sum() / N) if N else 0.0        # noqa: E731
        stats = np.array([N, mean(loss), mean(-surr), mean(lv), mean(H), mean((ratio - 1.0) - lr), mean(clipped.astype(np.float64)), 0.0])
    return dict(g_pi=g_pi, g_v=g_v, g_log_std=g_ls, stats=stats, ratio=ratio, clipped=clipped, vdiff=vdiff, vgap=vgap)


def kink_filter(inp, kind, clip=CLIP, vclip=VCLIP):
    """The inputs with mask cleared on the rows near a kink of the loss in float64 (a new dict; the tensors are shared but `mask`)."""
    ref = reference(inp, kind)
    r = ref["ratio"]
    near = (np.abs(r - (1 - clip)) < KINK) | (np.abs(r - (1 + clip)) < KINK) | (np.abs(ref["vdiff"] - vclip) < KINK)
    near |= (ref["vdiff"] > vclip) & (ref["vgap"] < KINK)
    out = dict(inp)
    out["mask"] = inp["mask"] * torch.from_numpy(~near).to(torch.uint8)
    return out


def ladder_figures(inp, kind, clip=CLIP):
    """(kept rows, rows with a ratio outside [1 - clip, 1 + clip], of those the clipped ones) of filtered inputs, in float64."""
    ref = reference(inp, kind)
    on = inp["mask"].numpy() != 0
    outside = on & ((ref["ratio"] < 1 - clip) | (ref["ratio"] > 1 + clip))
    return int(on.sum()), int(outside.sum()), int((outside & ref["clipped"]).sum())


@functools.lru_cache(maxsize=None)
def inputs(kind, rows, n, step=None):
    """(filtered inputs, step, masked rows before the filter) at the smallest step of LADDER that puts 5 % .. 60 % of the kept rows
    outside the clip interval (the last step if none does: the tests assert the conditions) -- or at the given step.  Read-only."""
    for step in (LADDER if step is None else (step,)):
        raw = build(kind, rows, n, step)
        inp = kink_filter(raw, kind)
        kept, outside, _ = ladder_figures(inp, kind)
        if 0.05 * kept <= outside <= 0.6 * kept:
            break
    return inp, step, int((raw["mask"] != 0).sum())


def torch_loss(inp, kind, dtype, vold=True, perm=None, clip=CLIP, vclip=VCLIP, tau=TAU, c_v=C_V, c_e=C_E):
    """The loss as a torch user writes it, on the CPU in `dtype`, with autograd from y, v and log_std -> dict of float64 numpy: g_pi, g_v
    (padded to 4 columns), g_log_std, stats[8] (N and the clipped share counted, the means computed in `dtype`).  perm: the rows in
    another order (another summation order of the same loss; the gradients come back in the original order)."""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
    if perm is not None:
        t = {k: (v if k == "log_std" else v[perm]) for k, v in t.items()}
    y, v = t["y"].clone().requires_grad_(), t["v"].clone().requires_grad_()
    ls = t["log_std"].clone().requires_grad_() if kind == "gaussian" else None
    w = (t["mask"] != 0).to(dtype)
    if kind == "categorical":
        lp = torch.log_softmax(y / tau, dim=-1)
        logp = lp.gather(-1, t["rec"].argmax(-1, keepdim=True)).squeeze(-1)
        ent = -(lp.exp() * lp).sum(-1)
    else:
        z = (t["rec"][..., :3] - y[..., :3]) * torch.exp(-ls)
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LOG_2PI
        ent = (ls + 0.5 * (1.0 + LOG_2PI)).sum(-1).expand_as(logp)
    lr = logp - t["logp_old"]
    ratio = torch.exp(lr)
    surr = torch.minimum(ratio * t["adv"], ratio.clamp(1 - clip, 1 + clip) * t["adv"])
    lv = (v - t["ret"]) ** 2
    if vold:
        vc = t["v_old"] + (v - t["v_old"]).clamp(-vclip, vclip)
        lv = torch.maximum(lv, (vc - t["ret"]) ** 2)
    lv = 0.5 * lv
    n = w.sum()
    pol, val, en = -(surr * w).sum() / n, (lv * w).sum() / n, (ent * w).sum() / n
    loss = pol + c_v * val - c_e * en
    loss.backward()
    with torch.no_grad():
        kl = (((ratio - 1.0) - lr) * w).sum() / n
        clipped = ((t["adv"] > 0) & (ratio > 1 + clip)) | ((t["adv"] < 0) & (ratio < 1 - clip))
        share = (clipped.to(dtype) * w).sum() / n
    g_pi, g_v = y.grad, torch.zeros_like(y.grad)
    g_v[..., 0] = v.grad
    if perm is not None:
        g_pi, g_v = g_pi[torch.argsort(perm)], g_v[torch.argsort(perm)]
    num = lambda x: x.detach().double().numpy()           # noqa: E731
    stats = np.array([float(n), float(loss.detach().double()), float(pol.detach().double()), float(val.detach().double()),
                      float(en.detach().double()), float(kl.double()), float(share.double()), 0.0])
    return dict(g_pi=num(g_pi), g_v=num(g_v), g_log_std=num(ls.grad) if ls is not None else None, stats=stats)


@functools.lru_cache(maxsize=None)
def case(kind, rows, n, vold, cut=None, step=None, perms=8):
    """(inputs, float64 reference, float32 yardstick, the yardstick's own error on stats [8] and g_log_std: the largest over the given
    order and `perms` permutations of the rows) of a shape of SHAPES, or of its first `cut` rows.  Computed once and shared: read-only."""
    inp, _, _ = inputs(kind, rows, n, step)
    if cut is not None:
        inp = head(inp, cut)
    ref = reference(inp, kind, vold)
    if ref["stats"][0] == 0:                    # no masked row: torch's mean is 0 / 0, the contract says all 0
        return inp, ref, ref, np.zeros(8), 0.0
    yard = torch_loss(inp, kind, torch.float32, vold)
    return (inp, ref, yard) + own_errors(inp, ref, kind, vold, perms)


def own_errors(inp, ref, kind, vold=True, perms=8, **par):
    """(e_stats [8], e_ls): the float32 yardstick's own error on the statistics and on g_log_std (0.0 for a categorical head), the
    largest over yardstick_util.row_orders; par: torch_loss' clip, vclip, tau, c_v, c_e."""
    e = Y.own_error(lambda order: torch_loss(inp, kind, torch.float32, vold, order, **par), ref, inp["adv"].shape[0], perms,
                    ("stats", "g_log_std")[:2 if kind == "gaussian" else 1])
    return e[0], float(e[1].max()) if kind == "gaussian" else 0.0


@functools.lru_cache(maxsize=None)
def factors():
    """{tensor: (mean factor, max factor)}: the project's (2, 4), or what profiles/ppo_head_float64.json records for a tensor (with why)."""
    return {k: Y.factor_of(Y.recorded(PROFILE, "factors"))(k) for k in ("g_pi", "g_v")}


def check(got, ref, yard, e_stats, e_ls, kind, what=""):
    """got: dict(g_pi, g_v, g_log_std, stats) of float64 numpy from the kernel.  Prints every figure, then asserts."""
    bad = Y.check_tensors([(k, got[k], ref[k], yard[k], factors()[k]) for k in ("g_pi", "g_v")], what)[1]
    if not (got["stats"][0] == ref["stats"][0] and got["stats"][7] == 0.0):
        bad.append("N")
    if ref["stats"][0] > 0 and abs(got["stats"][6] - ref["stats"][6]) > 1e-12:        # a count over N: the same rows are clipped (kinks left out)
        bad.append("clipped share")
    bad += Y.stats_out_of_bounds(got["stats"], ref["stats"], e_stats, STAT_NAMES, what)
    if kind == "gaussian":
        r = ref["g_log_std"]
        tol, err = Y.scalar_bound(r, e_ls), float(np.abs(got["g_log_std"] - r).max())
        print(f"{what} g_log_std: kernel error {err:.3e}, yardstick's own (9 row orders) {e_ls:.3e}, bound {tol:.3e}, max|g| {np.abs(r).max():.3e}")
        if not err <= tol:
            bad.append("g_log_std")
    assert not bad, (what, bad)
