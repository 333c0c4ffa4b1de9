"""What the tests of the centralised PPO critic (MAPPO: learner.joint_obs, PolicyRollout(central_critic=), PPOLearner on such a rollout)
share:

  join             bsx_ppo_joint_obs (include/battlespace_hip.h) restated in numpy: plane i's own observation, then its team-mates' in
                   ascending plane index; pure copies, so int32 views of float rows keep every bit
  central_rollout  ppo_learner_util.small_rollout with a central critic in place of the value head
  view, As         a central rollout (or its learner) under the names ppo_learner_util's harness reads -- value_actor, _value_w -- so
                   that keep / restore / everything / equal / allocates_nothing / members_are_identical are that file's own
  six_calls        one central minibatch from the raw calls; by_hand, the device update written out with them
  minibatch_float  a central minibatch in torch on the CPU, float64 (the restatement) or float32 (the yardstick): the two networks'
                   forwards, ppo_head_util's reference / torch_loss between them, the chain rule back through both networks
  first_step_meets_the_bars   ppo_learner_util's test of the first optimiser step, for two networks stepped and clipped on their own;
                   group_sums, the tied step's gradient in its float64 reference: every group's sum at each of its members
  critic_values    the critic on join(ro.obs), all T + 1 ticks, in torch on the CPU: float64 (what the recorded values are held to) or
                   float32 (the yardstick); value_yardstick_spread, how far the yardstick's own error moves when the join's columns and
                   w1's rows are permuted alike; PROFILE (profiles/mappo_wide.json), value_factors and append_ratios, what is recorded

Nothing here imports the native library at module level."""
import json
import os

import numpy as np
import torch

import actor_grad_util as G
import actor_ref_util as R
import adam_util as AU
import ppo_head_util as PH
import ppo_learner_util as L
import yardstick_util as Y
from ppo_learner_util import KW, STEPS, TAU

PARAMS = L.PARAMS
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mappo_wide.json")


def join(obs):
    """obs [..., A, Do] (any dtype: elements are copied) -> [..., A, n Do]: slot 0 = obs[..., i, :], slots 1 .. n-1 = the other planes of
    i's block of n adjacent columns in ascending index."""
    obs = np.asarray(obs)
    A, Do = obs.shape[-2:]
    n = A // 2
    out = np.empty((*obs.shape[:-2], A, n * Do), dtype=obs.dtype)
    for i in range(A):
        team, k = divmod(i, n)
        for s, j in enumerate([i] + [team * n + m for m in range(n) if m != k]):
            out[..., i, s * Do:(s + 1) * Do] = obs[..., j, :]
    return out


def join_bits(obs):
    """join on a float32 torch tensor through its int32 view -> int32 CPU tensor: NaN payloads and -0 are kept."""
    return torch.from_numpy(join(obs.detach().cpu().contiguous().view(torch.int32).numpy()))


class As:
    """obj under other names: the attributes given here first, every other one obj's."""

    def __init__(self, obj, **over):
        self.__dict__.update(_obj=obj, _over=over)

    def __getattr__(self, name):
        over = self.__dict__["_over"]
        return over[name] if name in over else getattr(self.__dict__["_obj"], name)


def view(ro):
    """A central rollout as ppo_learner_util reads a rollout: the critic as value_actor, its blob as _value_w."""
    return As(ro, value_actor=ro.central_critic, _value_w=ro._central_w)


def learner_view(learner):
    return As(learner, rollout=view(learner.rollout))


def central_rollout(kind, T=8, n=1, E=96, one_launch=False, opponent=None, chunk=None, group=1, auto_reset=True, normalize=False, seed=41,
                    runs=2, critic="central", capture=True):
    """ppo_learner_util.small_rollout's rollout with a central critic (critic="central"), its value head (critic="own") or no critic at
    all (critic=None): the same seeds, head weights scaled to trained size; group > 1: actor, critic and log_std tied before packing."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.learner import joint_width, tie_
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    A, D = 2 * n, 3 * n + 2
    cont = kind == "gaussian"
    torch.manual_seed(11)
    actor = StackedActor(A, D, 3 if cont else 4, device="cuda")
    net = StackedActor(A, joint_width(n) if critic == "central" else D, 1, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(60.0); net.w3.mul_(100.0)
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=auto_reset, continuous_actions=cont, device="cuda")
    env.reset()
    kw = dict(sample="gaussian", log_std=torch.full((A, 3), -0.5, device="cuda")) if cont else dict(sample="categorical", temperature=TAU)
    if group > 1:
        for x in (actor, net, kw.get("log_std")):
            if x is not None:
                tie_(x, group)
    if opponent is not None:
        mine, theirs = (env.possible_red, env.possible_blue) if opponent == "red" else (env.possible_blue, env.possible_red)
        kw["opponent"] = instinct.Team(mine, theirs, env)
    if critic is not None:
        kw["gae"] = dict(gamma=0.99, lam=0.95, normalize=normalize)
        kw.update(dict(central_critic=net, central_chunk=chunk) if critic == "central" else dict(value_actor=net))
    ro = PolicyRollout(env, actor, T, seed=3, one_launch=one_launch, chains=1, **kw)
    ro.start()
    if capture:
        ro.capture()
    for _ in range(runs):
        ro.run()
    torch.cuda.synchronize()
    return ro


def minibatch_of(ro, t0=0, t1=None, clone=False):
    """ticks [t0, t1) of a rollout's records as a learner.Minibatch of flat rows (clone: fresh allocations)."""
    from deep_rl_battlespace_amd.learner import Minibatch
    t1 = ro.T if t1 is None else t1
    flat = lambda x: (x[t0:t1].clone() if clone else x[t0:t1]).view(-1, *x.shape[2:])                      # noqa: E731
    return Minibatch(flat(ro.obs), flat(ro.scores), flat(ro.logp), flat(ro.adv), flat(ro.ret), flat(ro._mask), flat(ro.value))


def central_values(ro, blob=None):
    """ONE bsx_mlp_forward(raw=) of the critic packed in `blob` (default: the rollout's) over the join of ALL of ro.obs -> [T + 1, E, A]."""
    from deep_rl_battlespace_amd import _lib
    from deep_rl_battlespace_amd.learner import _mlp_forward, joint_obs
    T1, E, A, _ = ro.obs.shape
    x = joint_obs(ro.obs)
    y, v = torch.empty((T1 * E, A, 4), device="cuda"), torch.empty((T1 * E, A), device="cuda")
    _mlp_forward(_lib.load(), ro._central_w if blob is None else blob, x.view(T1 * E, A, -1), y, raw=v)
    torch.cuda.synchronize()
    return v.view(T1, E, A)


# ---------------------------------------------------------------------------------------------------- the sequence by hand
def six_calls(ro, kind, mb, blob_a, blob_v, head_kw):
    """One central minibatch from the raw calls -- the actor's forward without a value head, joint_obs, the critic's forward with raw,
    ppo_head(**head_kw) and both backward calls -- on the records `mb`, outputs and buffers of its own -> (actor row, critic row,
    g_log_std, stats)."""
    from deep_rl_battlespace_amd import _lib
    from deep_rl_battlespace_amd.learner import _actor_forward, _Buffers, _mlp_forward, _mlp_grad, joint_obs, ppo_head
    lib = _lib.load()
    (R_, A, D), dev = mb.obs.shape, mb.obs.device
    y, v, yv = torch.empty((R_, A, 4), device=dev), torch.empty((R_, A), device=dev), torch.empty((R_, A, 4), device=dev)
    _actor_forward(lib, blob_a, mb.obs, y)
    x = joint_obs(mb.obs)
    _mlp_forward(lib, blob_v, x, yv, raw=v)
    head = ppo_head(kind, y, v, mb.rec, mb.logp, mb.adv, mb.ret, mb.mask, temperature=TAU if kind == "categorical" else 1.0,
                    log_std=ro.log_std if kind == "gaussian" else None, v_old=mb.value, **head_kw)
    row_a = _mlp_grad(lib, _Buffers().get(R_, A, D, dev), blob_a, mb.obs, head.g_pi, True)
    row_v = _mlp_grad(lib, _Buffers().get(R_, A, x.shape[2], dev), blob_v, x, head.g_v, False)
    return row_a, row_v, head.g_log_std, head.stats


def everything(learner):
    """ppo_learner_util.everything of a central device_step learner, then the critic's own count and step statistics."""
    return L.everything(learner_view(learner)) + [learner.critic_step_count.clone(), learner.critic_step_stats.clone()]


def by_hand(ro, kind, rows_of, group=1):
    """STEPS optimiser steps on the rollout's own blobs: rows_of(i) -> (actor row, critic row, g_log_std, stats), then adam_step of the
    actor (and log_std) and mlp_adam_step of the critic, each from fresh moments and a zero count -> what everything() lists."""
    from deep_rl_battlespace_amd.learner import AdamState, adam_hyper, adam_step, mlp_adam_step
    sa, sv = AdamState(ro.actor), AdamState(ro.central_critic)
    ls_state = AdamState(ro.log_std) if kind == "gaussian" else None
    hyper = adam_hyper(KW["lr"], (0.9, 0.999), 1e-8, KW["max_grad_norm"])
    count, count_v = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    head_rows, step_rows, step_rows_v = [], [], []
    for i in range(STEPS):
        row_a, row_v, g_ls, st = rows_of(i)
        head_rows.append(st.clone())
        step_rows.append(adam_step([ro.actor], [row_a], [sa], [ro.fused.weights], hyper, count, log_std=ro.log_std if ls_state else None,
                                   g_log_std=g_ls, log_std_state=ls_state, group=group).clone())
        step_rows_v.append(mlp_adam_step([ro.central_critic], [row_v], [sv], [ro._central_w], hyper, count_v, group=group).clone())
    return L.keep(view(ro)) + [sa.m, sa.v, sv.m, sv.v] + ([ls_state.m, ls_state.v] if ls_state else []) + \
        [count, torch.stack(head_rows), torch.stack(step_rows), count_v, torch.stack(step_rows_v)]


# ---------------------------------------------------------------------------------------------------- the minibatch in torch
def head_inputs(ro, y, v, t0=0, t1=None):
    """ppo_head_util's input dict from a rollout's records of ticks [t0, t1) and the two networks' outputs y [R, A, 4], v [R, A] (CPU)."""
    mb = minibatch_of(ro, t0, t1)
    inp = dict(y=y, v=v, rec=mb.rec.cpu(), logp_old=mb.logp.cpu(), adv=mb.adv.cpu(), ret=mb.ret.cpu(), mask=mb.mask.cpu(), v_old=mb.value.cpu())
    if ro.log_std is not None:
        inp["log_std"] = ro.log_std.detach().cpu()
    return inp


def minibatch_float(ro, kind, dtype, mask=None, t0=0, t1=None):
    """A central minibatch over ticks [t0, t1) in torch on the CPU in `dtype` -> dict(actor, critic: {parameter: float64 array}, g_log_std,
    stats, y, v).  The forwards are StackedActor's own (the critic on join(obs)); between them stands ppo_head_util.reference (float64:
    the contract) or ppo_head_util.torch_loss (float32: what a torch user writes) at ppo_learner_util.KW's loss weights, which are that
    file's defaults; their g_pi and g_v go back through the two networks by the chain rule.  mask: the rows to keep, instead of the
    rollout's."""
    t1 = ro.T if t1 is None else t1
    obs = ro.obs[t0:t1].reshape(-1, *ro.obs.shape[2:]).cpu()
    x = torch.from_numpy(join(obs.numpy()))
    a, c = R.to(ro.actor, "cpu", dtype), R.to(ro.central_critic, "cpu", dtype)
    ya = a(obs.to(dtype))
    y = torch.cat([ya, torch.zeros((*ya.shape[:-1], 4 - ya.shape[-1]), dtype=dtype)], -1)
    v = c(x.to(dtype), squash=False)[..., 0]
    inp = head_inputs(ro, y.detach().float() if dtype == torch.float32 else y.detach(), v.detach().float() if dtype == torch.float32 else v.detach(),
                      t0, t1)
    if mask is not None:
        inp["mask"] = mask
    head = PH.reference(inp, kind) if dtype == torch.float64 else PH.torch_loss(inp, kind, torch.float32)
    ((y * torch.from_numpy(head["g_pi"]).to(dtype)).sum() + (v * torch.from_numpy(head["g_v"][..., 0]).to(dtype)).sum()).backward()
    grads = lambda m: {k: getattr(m, k).grad.double().numpy() for k in PARAMS}   # noqa: E731
    return dict(actor=grads(a), critic=grads(c), g_log_std=head["g_log_std"], stats=head["stats"], inp=inp, x=x)


def kept_rows(ro, kind, t0=0, t1=None):
    """The rollout's masked rows of ticks [t0, t1) away from every kink of the loss in float64 -- a hidden unit of the actor on obs or of
    the critic on join(obs) (actor_grad_util.near_kink), a ratio or a value difference at a clip boundary (ppo_head_util.kink_filter)
    -> (mask uint8 [R, A], the share of masked rows it drops)."""
    t1 = ro.T if t1 is None else t1
    obs = ro.obs[t0:t1].reshape(-1, *ro.obs.shape[2:]).cpu()
    x = torch.from_numpy(join(obs.numpy()))
    near = G.near_kink((ro.actor, obs), (ro.central_critic, x))
    with torch.no_grad():
        a, c = R.to_float64(ro.actor), R.to_float64(ro.central_critic)
        ya = a(obs.double())
        y = torch.cat([ya, torch.zeros((*ya.shape[:-1], 4 - ya.shape[-1]), dtype=torch.float64)], -1)
        inp = head_inputs(ro, y, c(x.double(), squash=False)[..., 0], t0, t1)
    masked = int((inp["mask"] != 0).sum())
    inp["mask"] = inp["mask"] * (~near).to(torch.uint8)
    mask = PH.kink_filter(inp, kind)["mask"]
    return mask, 1.0 - int((mask != 0).sum()) / max(masked, 1)


# ---------------------------------------------------------------------------------------------------- the first step
def group_sums(xs, g):
    """xs: arrays [A, ...] -> float64 copies with every group's sum (g adjacent agents) at each of its members: the tied step's
    gradient, one per group."""
    out = []
    for x in xs:
        x = np.asarray(x, np.float64)
        s = x.reshape(x.shape[0] // g, g, *x.shape[1:]).sum(1, keepdims=True)
        out.append(np.broadcast_to(s, (x.shape[0] // g, g, *x.shape[1:])).reshape(x.shape).copy())
    return out


def first_step_meets_the_bars(ro, kw, g=1, norm_rtol=1e-10):
    """ppo_learner_util.first_step_meets_the_bars for a central critic: one optimiser step from one start state on the same gradient
    rows -- PPOLearner's default path (install, clip_grad_norm_ once per network, torch Adam) and its device path (adam_step of the
    actor with log_std, mlp_adam_step of the critic) -- against adam_util.reference_step called ONCE PER NETWORK, each with its own
    norm and clip coefficient: that file's bars (adam_util.check_step: yardstick_util.FACTORS, pooled per network over the leaders'
    tensors).  The recorded norms and coefficients of step_stats / critic_step_stats are each network's own.  g > 1: the reference
    steps every group with the float64 sum of its members' rows."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    kw = dict(kw)
    hp = AU.hyper32(lr=3e-4, max_grad_norm=kw.pop("max_grad_norm", 0.5))
    kw = dict(KW, epochs=1, minibatches=1, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], max_grad_norm=hp["max_grad_norm"], **kw)
    rv = view(ro)
    start = L.keep(rv)
    device = PPOLearner(ro, device_step=True, **kw)
    rows = [r.clone() if r is not None else None for r in device.minibatch_grads(0, ro.T, pack=False)[:3]]
    gauss = ro.log_std is not None
    lead = lambda xs: [np.asarray(x)[::g] for x in xs]     # noqa: E731

    def arrays():
        torch.cuda.synchronize()
        return [AU.net_arrays(ro.actor) + ([ro.log_std.detach().cpu().numpy().copy()] if gauss else []), AU.net_arrays(ro.central_critic)]

    p0 = arrays()
    grads = [AU.row_to_tensors(rows[0].cpu().numpy(), ro.actor.n_actions) + ([rows[2].cpu().numpy()] if gauss else []),
             AU.row_to_tensors(rows[1].cpu().numpy(), 1)]
    ref = []
    for p, gr in zip(p0, grads):
        gs = group_sums(gr, g)
        zeros = [np.zeros_like(x, dtype=np.float64) for x in p]
        norm = float(np.sqrt(sum(float((x[::g] ** 2).sum()) for x in gs)))          # a group counts once in the norm: the leaders' sums
        coef = min(1.0, hp["max_grad_norm"] / (norm + 1e-6))
        P, M, V, _, _, _ = AU.reference_step(p, [coef * x for x in gs], zeros, zeros, 0, dict(hp, max_grad_norm=0.0))
        ref.append((P, M, V, norm, coef))
    device.update()
    got = arrays()
    moments = lambda st, na: AU.row_to_tensors(st.cpu().numpy(), na)     # noqa: E731
    got_m = [moments(device.adam_a.m, ro.actor.n_actions) + ([device.adam_ls.m.cpu().numpy()] if gauss else []), moments(device.adam_v.m, 1)]
    got_v = [moments(device.adam_a.v, ro.actor.n_actions) + ([device.adam_ls.v.cpu().numpy()] if gauss else []), moments(device.adam_v.v, 1)]
    figures = {}
    for name, st, (_, _, _, norm, coef) in (("actor", device.step_stats, ref[0]), ("critic", device.critic_step_stats, ref[1])):
        print(f"{name}: recorded norm {float(st[0, 1]):.9g} coefficient {float(st[0, 2]):.9g}; float64 {norm:.9g} {coef:.9g}")
        assert abs(float(st[0, 1]) - norm) <= norm_rtol * norm, name
        assert abs(float(st[0, 2]) - coef) <= max(norm_rtol, 1e-6) * coef, name
        figures[name] = (norm, coef)
    assert L.members_are_identical(learner_view(device), g) is None
    L.restore(rv, start)
    default = PPOLearner(ro, **kw)
    assert all(torch.equal(a, b) for a, b in zip(default.minibatch_grads(0, ro.T)[:2], rows))      # the same gradient rows, bit for bit
    default.update()
    torch.cuda.synchronize()
    assert L.blobs_are_packs(rv)
    for t_ in L.shared(rv):
        v = t_.detach().view(t_.shape[0] // g, g, -1)
        assert torch.equal(v, v[:, :1].expand_as(v))
    tor = arrays()
    state = lambda key: [[default.optimizer.state[getattr(net, k)][key].cpu().numpy() for k in PARAMS] for net in (ro.actor, ro.central_critic)]     # noqa: E731
    tor_m, tor_v = state("exp_avg"), state("exp_avg_sq")
    if gauss:
        tor_m[0].append(default.optimizer.state[ro.log_std]["exp_avg"].cpu().numpy())
        tor_v[0].append(default.optimizer.state[ro.log_std]["exp_avg_sq"].cpu().numpy())
    for i in range(2):
        pmv = lambda p, m, v: dict(p=lead(p), m=lead(m), v=lead(v))     # noqa: E731
        AU.check_step(pmv(got[i], got_m[i], got_v[i]), pmv(*ref[i][:3]), pmv(tor[i], tor_m[i], tor_v[i]), f"net{i}", names=("p", "m", "v"))
    return figures


# ---------------------------------------------------------------------------------------------------- the recorded values
# the recorded values against float64: (kind, n, one_launch) at VALUE_E games (ragged against a wave) -- every join width, 5, 16, 33, 56
VALUE_E = 33
VALUE_CASES = {
    "categorical-n1": ("categorical", 1, False),
    "gaussian-n2": ("gaussian", 2, False),
    "categorical-n3": ("categorical", 3, False),
    "gaussian-n4": ("gaussian", 4, False),
    "categorical-n4-one_launch": ("categorical", 4, True),
}


def critic_values(ro, dtype, perm=None):
    """The critic of a central rollout on join(ro.obs), all T + 1 ticks, in torch on the CPU in `dtype` (StackedActor's own forward,
    the raw head) -> float64 array [T + 1, E, A].  perm: a permutation of the join's columns, applied to the columns of x and to the rows
    of w1 alike -- the same function of the same inputs, every sum of the first layer taken in another order."""
    T1, E, A, _ = ro.obs.shape
    x = torch.from_numpy(join(ro.obs.detach().cpu().numpy())).view(T1 * E, A, -1)
    c = R.to(ro.central_critic, "cpu", dtype)
    with torch.no_grad():
        if perm is not None:
            perm = torch.as_tensor(perm)
            x = x[..., perm].contiguous()
            c.w1.copy_(c.w1[:, perm, :].clone())
        return c(x.to(dtype), squash=False)[..., 0].double().numpy().reshape(T1, E, A)


def value_yardstick_spread(ro, ref, yard, perms=8):
    """(max ratio, mean ratio): how far max and mean |yard - ref| of the float32 yardstick move over `perms` seeded column permutations
    of critic_values (actor_grad_util.spread: the larger of p / base and base / p).  No kernel output enters."""
    W = ro.central_critic.obs_len
    others = ({"v": critic_values(ro, torch.float32, torch.randperm(W, generator=torch.Generator().manual_seed(4100 + p)))} for p in range(perms))
    return G.spread({"v": ref}, {"v": yard}, others, ("v",))["v"]


def value_factors(case, profile=None):
    """(fm, fx) of a case of the recorded-values test: the exception profiles/mappo_wide.json records for it, else yardstick_util.FACTORS."""
    return Y.factor_of(Y.recorded(PROFILE if profile is None else profile, "exceptions", case))("values")


def append_ratios(case, ratios, spread):
    """Appends a case's measured ratios and yardstick spread to the file BSX_MAPPO_RATIOS_OUT names, if it names one."""
    path = os.environ.get("BSX_MAPPO_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "ratios": [round(float(r), 4) for r in ratios], "yardstick_spread_max_mean": [round(float(s), 4) for s in spread]}) + "\n")
