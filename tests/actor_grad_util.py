"""What the tests of the actor's fused training pass (learner.fused_apply, csrc/bsx_actor_grad.hip) share:

  CASES            (class, n, outputs, squash) on the input classes of actor_ref_util, team sizes 1 .. 16; LARGE: (n, rows) with many rows
  plan             workgroups per agent and rounds of a launch at (rows, A, D), from the library's own workspace size
  reference        per case, cached: the float64 autograd gradients g64 (torch on the CPU, loss = (y * go).sum()), the float32 ones g32 of
                   the same network (the yardstick: what float32 itself loses on these inputs), the upstream gradient go and the share of
                   rows it leaves out
  kink_free_go     go with the ReLU kinks left out BY CONSTRUCTION: a hidden unit whose post-LayerNorm value is within rounding of 0 flips
                   its mask between float32 and float64 and moves a summed gradient by a whole row's contribution (~1/R of the sum, against
                   ~1e-7 for rounding), so go = 0 on every row (e, a) where, in float64, any of the 128 post-LayerNorm pre-ReLU values has
                   |y| < 1e-4.  The same go feeds the reference, the yardstick and the kernel
  spread / row_permutation_spread / permutation_spread   how far the yardstick's own error moves under an equivalent float32
                   evaluation: the accumulator, the rows summed in another order, and the latter for a case of this file
  factors / check  the bound: yardstick_util's per-tensor bars, with (fm, fx) = the project's (2, 4) (yardstick_util.FACTORS)
                   except where the recorded spread of the yardstick reaches them (profiles/actor_grad_float64.json says where and why)
  CLIP, TAU, _to, _logp, _ppo, _ppo_own_error   the PPO loss in torch (clipped surrogate + value loss - entropy bonus over the kept rows of a rollout
                   record) that tests/test_hip_actor_grad.py and tests/test_hip_ppo_learner.py both hold the fused paths to

plan, autograd_grads (with the input's gradient as an eleventh tensor "x" on request), spread, row_permutation_spread and check
are the one yardstick of every fused-gradient test: tests/mlp_grad_util.py brings its own cases and factors and imports these.
Nothing here imports the native library but plan() and the fused legs of _logp and _ppo."""
import functools
import os

import numpy as np
import torch

import actor_ref_util as R
import yardstick_util as Y

PARAMS = R.PARAMS
KINK = 1e-4
KINK_CAP = 0.05
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "actor_grad_float64.json")

# (class, n, outputs, squash).  Left out, seed 0: dead_half at n = 3 (one agent's constant all -1 row has a kink unit: 57.6 % of its rows would go),
# fresh at n = 3 (15.4 % for the same reason) and fresh at n = 13 and n = 16 (15.1 % for the same reason: the wide teams below n = 12 are fresh,
# the ones above trained_like).  The rest stay below KINK_CAP, which test_actor_grad_cpu.py checks.
# Team sizes 5 .. 10 reach D = 3n + 2 = 17, 26 and 32 (the 32-column x image with little or no zero padding); n >= 11 has D > 32 and takes the
# kernel's two-tile dW1 form (D = 35, 41, 50).  With 512 / (2n) workgroups per agent at most, the dense row count makes the workgroups of
# n = 8, 10, 11 go round their tile loop twice and those of n = 13, 16 three times (MULTI_ROUND; test_actor_grad_cpu.py derives it from
# the workspace size, so that a change of the cap cannot quietly turn these back into one-round cases).
CASES = (("fresh", 1, 4, True), ("fresh", 4, 4, True), ("shipped", 2, 4, True), ("trained_like", 1, 4, True),
         ("trained_like", 4, 4, True), ("trained_like", 3, 3, True), ("fresh", 2, 3, True), ("flat_rows", 2, 4, True), ("wide_obs", 2, 4, True),
         ("dead_half", 1, 4, True), ("fresh", 1, 1, False), ("trained_like", 3, 1, False),
         ("fresh", 5, 4, True), ("fresh", 8, 4, True), ("fresh", 10, 4, True), ("fresh", 11, 4, True), ("trained_like", 11, 3, True),
         ("trained_like", 13, 1, False), ("trained_like", 16, 4, True), ("trained_like", 16, 1, False))
MULTI_ROUND = tuple(c for c in CASES if c[1] >= 8)
# (n, rows) of the regime the kernel was written for, at small teams: many rows, the workgroup cap reached, two rounds.  (1, 33 000) has 1 032
# tiles on 256 workgroups per agent (the merge kernel's widest input); the last round of both is nearly empty: most waves lie beyond R.
LARGE = ((1, 33000), (4, 8300))


def plan(rows, A, D):
    """(workgroups per agent P, rounds) of bsx_mlp_grad at (rows, A, D) -- bsx_actor_grad at (rows, n) is (rows, 2n, 3n + 2) --, P read
    back from the workspace size the library asks for."""
    import ctypes
    from deep_rl_battlespace_amd import _lib
    nb = _lib.c_size_t()
    _lib.check(_lib.load().bsx_mlp_grad_workspace_bytes(rows, A, D, ctypes.byref(nb)), "bsx_mlp_grad_workspace_bytes")
    G = 64 * D + 4096 + 6 * 64 + 260
    assert nb.value % (A * G * 4) == 0
    P = nb.value // (A * G * 4)
    tiles = (rows + 31) // 32
    return P, (tiles + 4 * P - 1) // (4 * P)


def case_id(case):
    return "%s-n%d-out%d-%s" % (case[0], case[1], case[2], "tanh" if case[3] else "raw")


def with_outputs(actor, outputs):
    """The actor with its head cut (or kept) to `outputs` columns: the body is the class's own."""
    if actor.n_actions == outputs:
        return actor
    a = R._new(actor.n_actors, actor.obs_len, outputs)
    with torch.no_grad():
        for k in R.BODY:
            getattr(a, k).copy_(getattr(actor, k))
        a.w3.copy_(actor.w3[:, :, :outputs]); a.b3.copy_(actor.b3[:, :, :outputs])
    return a


def pre_relu64(actor, obs):
    """float64 [A, R, 128]: the post-LayerNorm, pre-ReLU values of both hidden layers."""
    a = R.to_float64(actor)
    with torch.no_grad():
        x = obs.detach().cpu().double().transpose(0, 1)
        y1 = a._ln(torch.baddbmm(a.b1, x, a.w1), a.g1, a.h1)
        y2 = a._ln(torch.baddbmm(a.b2, torch.relu(y1), a.w2), a.g2, a.h2)
    return torch.cat([y1, y2], -1)


def near_kink(*evaluations):
    """bool [R, A]: where, in float64, a hidden unit of any of the (network, input [R, A, D]) pairs is within KINK of its ReLU's kink."""
    return functools.reduce(torch.logical_or, ((pre_relu64(net, x).abs() < KINK).any(-1) for net, x in evaluations)).transpose(0, 1)


def kink_free_go(actor, obs, seed=0):
    """(go float32 [R, A, outputs], share [A]): standard normals, 0 on the rows with a hidden unit within KINK of its ReLU's kink."""
    near = near_kink((actor, obs))
    g = torch.Generator().manual_seed(3000 + seed)
    go = torch.randn((obs.shape[0], actor.n_actors, actor.n_actions), generator=g)
    go[near] = 0.0
    return go, near.double().mean(0).numpy()


def autograd_grads(net, x, go, squash, dtype, input_grad=False):
    """{name: float64 array}: d (y * go).sum() / d parameter, torch autograd on the CPU in `dtype`; input_grad: and d / d x, as "x"."""
    a = R.to_float64(net) if dtype == torch.float64 else R.to_cpu32(net)
    xx = x.detach().cpu().to(dtype).requires_grad_(input_grad)
    (a(xx, squash=squash) * go.to(dtype)).sum().backward()
    out = {k: getattr(a, k).grad.double().numpy() for k in PARAMS}
    if input_grad:
        out["x"] = xx.grad.double().numpy()
    return out


def build_case(case, rows=None, seed=0):
    cls, n, outputs, squash = case
    actor, obs = R.CLASSES[cls](n, seed)
    actor = with_outputs(actor, outputs)
    if rows is not None:
        obs = obs[:rows].contiguous()
    go, share = kink_free_go(actor, obs, seed)
    return actor, obs, go, share


@functools.lru_cache(maxsize=None)
def reference(case, rows=None):
    """(actor, obs, go, g64, g32, share) of a case, computed once and shared: treat every part as read-only."""
    actor, obs, go, share = build_case(case, rows)
    g64 = autograd_grads(actor, obs, go, case[3], torch.float64)
    g32 = autograd_grads(actor, obs, go, case[3], torch.float32)
    return actor, obs, go, g64, g32, share


@functools.lru_cache(maxsize=None)
def reference_large(n, rows, seed=0):
    """The same tuple for a LARGE pair: the fresh class's actor on `rows` of its observations (uniform, every seventh row all -1)."""
    actor = R._fresh_actor(n, 10 + n + seed)
    obs = R._uniform_obs(n, seed, E=rows)
    obs[::7] = -1.0
    go, share = kink_free_go(actor, obs, seed)
    g64 = autograd_grads(actor, obs, go, True, torch.float64)
    g32 = autograd_grads(actor, obs, go, True, torch.float32)
    return actor, obs, go, g64, g32, share


def spread(g64, g32, others, names=PARAMS):
    """{name: (max ratio, mean ratio)}: how far max(e_t) and mean(e_t) of the float32 yardstick g32 move over `others`, equivalent
    float32 evaluations of the same gradients (the larger of p / base and base / p; an error of exactly 0 on either side is skipped)."""
    out = {k: [1.0, 1.0] for k in names}
    for gp in others:
        for k in names:
            e0, e1 = np.abs(g32[k] - g64[k]), np.abs(gp[k] - g64[k])
            for i, f in enumerate((np.max, np.mean)):
                a, b = float(f(e0)), float(f(e1))
                if a > 0 and b > 0:
                    out[k][i] = max(out[k][i], a / b, b / a)
    return {k: tuple(v) for k, v in out.items()}


def row_permutation_spread(net, x, go, g64, g32, squash, names=PARAMS, perms=8):
    """spread over `perms` orders of the rows (yardstick_util.row_orders): the same network, the same rows, another summation order.
    With "x" in `names` the input's gradient is compared row by row."""
    def permuted(idx):
        gp = autograd_grads(net, x[idx].contiguous(), go[idx].contiguous(), squash, torch.float32, "x" in names)
        if "x" in names:
            gp["x"] = gp["x"][torch.argsort(idx).numpy()]
        return gp
    return spread(g64, g32, (permuted(idx) for idx in list(Y.row_orders(x.shape[0], perms))[1:]), names)


def permutation_spread(case, perms=8):
    """row_permutation_spread of `case`: one of CASES, or a reference tuple."""
    actor, obs, go, g64, g32, _ = reference(case) if isinstance(case[0], str) else case
    return row_permutation_spread(actor, obs, go, g64, g32, case[3] if isinstance(case[0], str) else True, PARAMS, perms)


@functools.lru_cache(maxsize=None)
def factors():
    """{name: (mean factor, max factor)} from profiles/actor_grad_float64.json."""
    return {k: Y.factor_of(Y.recorded(PROFILE, "factors"))(k) for k in PARAMS}


def check(got, g64, g32, what="", names=PARAMS, factor_of=None):
    """Every tensor of `names` within its factors (fm, fx) = factor_of(name) of the yardstick's error -- the actor's recorded factors()
    unless the caller brings its own; prints the figures first.  Returns the ratios."""
    r, bad = Y.check_tensors([(k, got[k], g64[k], g32[k], (factor_of or factors().__getitem__)(k)) for k in names], what, "ratios")
    assert not bad, (what, [(k, r[k]) for k in bad])
    return r


# ---------------------------------------------------------------------------------------------------- the PPO loss, in torch
TAU, CLIP = 0.7, 0.2


def _to(actor, device="cuda", dtype=torch.float32):
    return R.to(actor, device, dtype)


def _logp(actor, ls, obs, act, kind, fused):
    from deep_rl_battlespace_amd.learner import categorical_log_prob
    from deep_rl_battlespace_amd.rollout import gaussian_log_prob
    if kind == "gaussian":
        return gaussian_log_prob(actor, ls, obs, act, fused=fused)
    return categorical_log_prob(actor, obs, act, temperature=TAU, fused=fused)


def _ppo(actor, critic, ls, rec, keep, kind, fused, device, dtype, perm=None):
    """(loss, actor grads, critic grads, log_std grad) of the clipped surrogate + value loss - entropy bonus over the kept rows, the rows
    flattened (and permuted: another summation order of the same loss)."""
    from deep_rl_battlespace_amd.learner import fused_apply
    a, c = _to(actor, device, dtype), _to(critic, device, dtype)
    l = ls.detach().to(device=device, dtype=dtype).requires_grad_() if ls is not None else None
    A, D = rec["obs"].shape[-2:]
    flat = dict(obs=rec["obs"].reshape(-1, A, D), act=rec["act"].reshape(-1, A, *rec["act"].shape[3:]), logp=rec["logp"].reshape(-1, A),
                adv=rec["adv"].reshape(-1, A), ret=rec["ret"].reshape(-1, A), keep=keep.reshape(-1, A))
    if perm is not None:
        flat = {k: v[perm] for k, v in flat.items()}
    f = {k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)).contiguous() for k, v in flat.items()}
    logp, ent = _logp(a, l, f["obs"], f["act"], kind, fused)
    v = fused_apply(c, f["obs"], squash=False)[..., 0] if fused else c(f["obs"], squash=False)[..., 0]
    ratio = torch.exp(logp - f["logp"])
    surr = torch.minimum(ratio * f["adv"], ratio.clamp(1 - CLIP, 1 + CLIP) * f["adv"])
    w = f["keep"].to(dtype)
    loss = (-(surr * w).sum() + 0.5 * ((v - f["ret"]) ** 2 * w).sum() - 0.01 * (ent * w).sum()) / w.sum()
    loss.backward()
    grads = lambda m: {k: getattr(m, k).grad.double().cpu().numpy() for k in PARAMS}   # noqa: E731
    return float(loss.detach().double()), grads(a), grads(c), (l.grad.double().cpu().numpy() if l is not None else None), ratio.detach().double().cpu()


def nudge(net, scale, seed=5):
    """Every parameter moved by scale * mean|p| * a standard normal (drawn on the CPU: the same step on every device)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in PARAMS:
            p = getattr(net, k)
            p.add_((scale * p.abs().mean().cpu() * torch.randn(p.shape, generator=g)).to(p.device))


def _ppo_ladder(actor0, critic, ls, rec, kind, cols=None):
    """The learner's policy a step away from the one that played (actor0 nudged), so that ratios leave 1 and some are clipped: the
    smallest step of a fixed ladder that clips 5 % .. 60 % of the kept rows, chosen on the float64 reference alone.  Rows kept: the
    agents' own decisions (mask; of the agent columns `cols` only: a scripted team's are not) away from every kink of the loss in float64
    -- a hidden unit of either network or a ratio within KINK of a kink -- the same in every path.  -> (actor, critic, ls on the CPU,
    keep [T, E, A], the figures)."""
    critic, ls = _to(critic, "cpu"), (ls.cpu() if ls is not None else None)
    T, E, A, D = rec["obs"].shape
    flat_obs = rec["obs"].reshape(-1, A, D)
    on = torch.zeros(A, dtype=torch.bool)
    on[list(range(A)) if cols is None else cols] = True
    masked = rec["mask"] & on
    for scale in (0.03, 0.06, 0.12, 0.25, 0.5, 1.0):
        actor = _to(actor0, "cpu")
        nudge(actor, scale)
        near = near_kink((actor, flat_obs), (critic, flat_obs)).reshape(T, E, A)
        keep = masked & ~near
        r64 = _ppo(actor, critic, ls, rec, keep, kind, False, "cpu", torch.float64)[4].reshape(T, E, A)
        keep = keep & ((r64 - (1 - CLIP)).abs() > KINK) & ((r64 - (1 + CLIP)).abs() > KINK)
        kept, clipped = int(keep.sum()), int((keep & ((r64 < 1 - CLIP) | (r64 > 1 + CLIP))).sum())
        kink = float((masked & near).sum()) / max(int(masked.sum()), 1)
        print(kind, "step", scale, "rows kept", kept, "of", int(masked.sum()), "masked; clipped", clipped)
        if 0.05 * kept <= clipped <= 0.6 * kept:
            break
    return actor, critic, ls, keep, dict(step=scale, masked=int(masked.sum()), kept=kept, clipped=clipped, kink_share=kink)


def _ppo_own_error(actor, critic, ls, rec, keep, kind, L64, l64):
    """What the torch path itself loses on a record: _ppo in float32 on the GPU over yardstick_util.row_orders of the flattened rows,
    against the float64 loss L64 and log_std gradient l64 -> (the loss in the given order, yardstick_util.scalar_bound of its largest
    error, the largest error of log_std's gradient or 0.0 without one)."""
    runs = [_ppo(actor, critic, ls, rec, keep, kind, False, "cuda", torch.float32, order) for order in Y.row_orders(keep[..., 0].numel())]
    return runs[0][0], Y.scalar_bound(L64, max(abs(r[0] - L64) for r in runs)), (max(abs(r[3] - l64).max() for r in runs) if ls is not None else 0.0)
