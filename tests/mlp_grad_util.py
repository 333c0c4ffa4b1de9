"""What the tests of the fused MLP on any input width and of its input gradient (learner.fused_mlp / mlp_grad, bsx_mlp_forward /
bsx_mlp_grad) share:

  TABLE / CASES    (A, D, outputs, squash, rows) at the smallest sizes each mechanism can go wrong at, each on a freshly initialised
                   network and on one whose LayerNorm gains and biases are moved off 1 / 0
  build / reference   per case, cached: the network, x uniform in [-1, 1], a kink-free go (actor_grad_util.kink_free_go: 0 on every row
                   where, in float64, a pre-ReLU value is within 1e-4 of 0), the float64 autograd gradients of (y * go).sum() in the ten
                   parameters AND in x (torch on the CPU), the float32 ones of the same (the yardstick), the share of rows left out
  check            actor_grad_util's, with x as an eleventh tensor: mean(e_k) <= fm mean(e_t), max(e_k) <= fx max(e_t),
                   (fm, fx) = yardstick_util.FACTORS = (2, 4) for every tensor, except where the recorded spread of the yardstick
                   itself reaches them (factors: profiles/mlp_input_grad.json says where and why)
  unit_permutation_spread   how far the yardstick's own error moves when the SAME network is written with its hidden units in another
                   order (another summation order of the same float32 sums): the spread a one-row case has, where no row order exists
  row_permutation_spread    the same under another order of the rows (actor_grad_util.row_permutation_spread): what moves b3
  factor_rule      yardstick_util's: the rule that turns a recorded spread into factors (tools/measure_mlp_grad.py writes what it gives)
  plan / spread    actor_grad_util's: workgroups per agent and rounds of a bsx_mlp_grad launch; the spread accumulator
  ddpg_case        one DDPG step at 1v1: actor 5 -> 4, critic 9 -> 1, 96 rows, the row weights w that leave both networks' kinks out

Nothing here imports the native library but plan()."""
import functools
import os

import torch

import actor_grad_util as U
import actor_ref_util as R
import yardstick_util as Y

PARAMS = U.PARAMS
TENSORS = PARAMS + ("x",)
(FM, FX), factor_rule = Y.FACTORS, Y.factor_rule
KINK_CAP, plan, spread = U.KINK_CAP, U.plan, U.spread
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlp_input_grad.json")

# (A, D, outputs, squash, row counts): what each line reaches is said in the comment behind it
TABLE = ((1, 1, 1, False, (1,)),                                   # least of everything; one valid lane
         (2, 5, 4, True, (129,)),                                  # 1v1 actor; odd D (pad column 5)
         (2, 9, 1, False, (1, 31, 32, 33, 127, 128, 129)),         # 1v1 Q critic; tile and workgroup edges
         (4, 24, 1, False, (161,)),                                # the reference's 2v2 critic
         (3, 32, 3, True, (129,)),                                 # a full single x tile; odd A
         (3, 33, 1, False, (129,)),                                # first two-tile (MT1 = 2) case; odd D
         (2, 64, 4, True, (129,)),                                 # full width
         (32, 54, 1, False, (2100,)))                              # two rounds: 16 workgroups x 128 rows = 2048 < 2100
VARIANTS = ("fresh", "gains")
CASES = tuple((A, D, na, sq, rows, var) for A, D, na, sq, rr in TABLE for rows in rr for var in VARIANTS)


def case_id(case):
    A, D, na, sq, rows, var = case
    return "A%d-D%d-out%d-%s-R%d-%s" % (A, D, na, "tanh" if sq else "raw", rows, var)


def make_net(A, D, na, variant, seed=0):
    """A freshly initialised StackedActor on the CPU; variant "gains": LayerNorm gains in [0.5, 1.5], biases in [-0.2, 0.2]."""
    torch.manual_seed(1000 * seed + 97 * A + D)
    net = R._new(A, D, na)
    if variant == "gains":
        g = torch.Generator().manual_seed(7000 + seed)
        with torch.no_grad():
            for k in ("g1", "g2"):
                getattr(net, k).add_(torch.rand(getattr(net, k).shape, generator=g) - 0.5)
            for k in ("h1", "h2"):
                getattr(net, k).add_(0.4 * torch.rand(getattr(net, k).shape, generator=g) - 0.2)
    return net


def uniform_x(rows, A, D, seed=0):
    return torch.rand((rows, A, D), generator=torch.Generator().manual_seed(2000 + seed + 31 * rows)) * 2 - 1


def build(case, seed=0):
    A, D, na, sq, rows, var = case
    net, x = make_net(A, D, na, var, seed), uniform_x(rows, A, D, seed)
    go, share = U.kink_free_go(net, x, seed)
    return net, x, go, share


autograd_grads = functools.partial(U.autograd_grads, input_grad=True)        # the ten parameters' gradients and "x", the input's


@functools.lru_cache(maxsize=None)
def reference(case):
    """(net, x, go, g64, g32, share) of a case, computed once and shared: treat every part as read-only."""
    net, x, go, share = build(case)
    return net, x, go, autograd_grads(net, x, go, case[3], torch.float64), autograd_grads(net, x, go, case[3], torch.float32), share


def unit_permutation_spread(case, perms=8):
    """{tensor: (max ratio, mean ratio)}: over `perms` orders of the 64 + 64 hidden units (the same function of x, every sum over units
    taken in another order), how far max(e_t) and mean(e_t) of the float32 yardstick move from the unpermuted one (the larger of p / base
    and base / p).  No kernel output enters."""
    net, x, go, g64, g32, _ = reference(case)

    def permuted(p):
        g = torch.Generator().manual_seed(6000 + p)
        p1, p2 = torch.randperm(64, generator=g), torch.randperm(64, generator=g)
        q1, q2 = torch.argsort(p1), torch.argsort(p2)
        m = R._new(net.n_actors, net.obs_len, net.n_actions)
        with torch.no_grad():
            m.w1.copy_(net.w1[:, :, p1]); m.w2.copy_(net.w2[:, p1][:, :, p2]); m.w3.copy_(net.w3[:, p2])
            for k, pp in (("b1", p1), ("g1", p1), ("h1", p1), ("b2", p2), ("g2", p2), ("h2", p2)):
                getattr(m, k).copy_(getattr(net, k)[:, :, pp])
            m.b3.copy_(net.b3)
        gp = autograd_grads(m, x, go, case[3], torch.float32)
        back = dict(gp)                                            # the gradients of the permuted network, back in the original order
        back["w1"] = gp["w1"][:, :, q1]; back["w2"] = gp["w2"][:, q1][:, :, q2]; back["w3"] = gp["w3"][:, q2]
        for k, qq in (("b1", q1), ("g1", q1), ("h1", q1), ("b2", q2), ("g2", q2), ("h2", q2)):
            back[k] = gp[k][:, :, qq]
        return back
    return spread(g64, g32, (permuted(p) for p in range(perms)), TENSORS)


def row_permutation_spread(case, perms=8):
    """{tensor: (max ratio, mean ratio)}: the same under `perms` orders of the ROWS (actor_grad_util.row_permutation_spread: its method
    and seeds): what moves a sum over rows such as b3, which has one value per agent and output.  x's gradient is compared row by row."""
    net, x, go, g64, g32, _ = reference(case)
    return U.row_permutation_spread(net, x, go, g64, g32, case[3], TENSORS, perms)


def exceptions_from(spreads):
    """{case id or "*": {tensor: [fm, fx]}} from {source: {case id: {tensor: [max ratio, mean ratio]}}}: yardstick_util.exceptions_from
    on, per case and tensor, the largest recorded spread over the sources."""
    return Y.exceptions_from({cid: {k: [max(s[cid][k][i] for s in spreads.values()) for i in (0, 1)] for k in TENSORS}
                              for cid in map(case_id, CASES)})


@functools.lru_cache(maxsize=None)
def factors():
    """{case id or "*": {tensor: (fm, fx)}}: the exceptions recorded in profiles/mlp_input_grad.json; everything else is (FM, FX)."""
    return {cid: {k: tuple(v) for k, v in t.items()} for cid, t in Y.recorded(PROFILE, "factors", "exceptions").items()}


def check(got, g64, g32, what="", names=TENSORS, cid=None):
    """actor_grad_util.check with case `cid`'s factors: its recorded exception, the one under "*", or (FM, FX).  Returns the ratios."""
    return U.check(got, g64, g32, what, names, Y.factor_of(factors().get(cid, {}), factors().get("*", {})))


# ------------------------------------------------------------------------------------------------ one DDPG step
DDPG = dict(A=2, Da=5, Dc=9, rows=96)


@functools.lru_cache(maxsize=None)
def ddpg_case(seed=0):
    """(actor, critic, obs, act, target, w, share): a 1v1 actor (5 -> 4, tanh) and Q critic (obs (+) action: 9 -> 1), 96 rows; act are
    the replayed actions of the critic loss, target its fixed TD targets; w [R, A]: standard normal row weights, 0 on the rows where, in
    float64, either network has a pre-ReLU value within 1e-4 of 0 -- the critic at obs (+) act and at obs (+) pi(obs), the actor at
    obs; share: the part of the rows left out."""
    A, Da, Dc, rows = DDPG["A"], DDPG["Da"], DDPG["Dc"], DDPG["rows"]
    actor, critic = make_net(A, Da, 4, "gains", seed + 1), make_net(A, Dc, 1, "gains", seed + 2)
    with torch.no_grad():
        critic.w3.mul_(100.0); actor.w3.mul_(60.0)                # head sums of order 1, as after some training
    g = torch.Generator().manual_seed(5000 + seed)
    obs = torch.rand((rows, A, Da), generator=g) * 2 - 1
    act = torch.rand((rows, A, 4), generator=g) * 2 - 1
    target = torch.randn((rows, A), generator=g)
    with torch.no_grad():
        pi = R.to_float64(actor)(obs.double())
    near = U.near_kink((actor, obs), (critic, torch.cat([obs, act], -1)), (critic, torch.cat([obs.double(), pi], -1)))
    w = torch.randn((rows, A), generator=g)
    w[near] = 0.0
    return actor, critic, obs, act, target, w, float(near.double().mean())


def ddpg_losses(actor, critic, obs, act, target, w, apply):
    """(actor loss, critic loss) with apply(net, x, squash) as the network: -(w Q(obs (+) pi(obs))).sum() and the weighted TD loss
    0.5 (w (Q(obs (+) act) - target)^2).sum()."""
    q_pi = apply(critic, torch.cat([obs, apply(actor, obs, True)], -1), False)[..., 0]
    q = apply(critic, torch.cat([obs, act], -1), False)[..., 0]
    return -(w * q_pi).sum(), 0.5 * (w * (q - target) ** 2).sum()


def ddpg_grads(actor, critic, obs, act, target, w, dtype, device="cpu", apply=None):
    """({actor tensor: grad}, {critic tensor: grad}) as float64 arrays: the actor's ten gradients of the actor loss (they come through the
    critic's INPUT gradient) and the critic's ten of the critic loss."""
    a, c = U._to(actor, device, dtype), U._to(critic, device, dtype)
    t = [v.to(device=device, dtype=dtype) for v in (obs, act, target, w)]
    la, lc = ddpg_losses(a, c, *t, apply or (lambda net, x, squash: net(x, squash=squash)))
    ga = torch.autograd.grad(la, [getattr(a, k) for k in PARAMS], retain_graph=True)
    gc = torch.autograd.grad(lc, [getattr(c, k) for k in PARAMS])
    num = lambda gs: {k: g.double().cpu().numpy() for k, g in zip(PARAMS, gs)}     # noqa: E731
    return num(ga), num(gc)
