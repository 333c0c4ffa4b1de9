"""The small rollout the PPO learner's GPU tests share (by default the record of tests/test_hip_actor_grad.py's PPO test: n = 1, E = 96,
T = 8, the graph form, no opponent, head weights scaled to trained size), built fresh for each caller: the tests move its networks."""
import torch

PARAMS = ("w1", "b1", "g1", "h1", "w2", "b2", "g2", "h2", "w3", "b3")
TAU = 0.7


def small_rollout(kind, gae=True, sample=True, T=8, n=1, E=96, one_launch=False, chains=1, opponent=None, normalize=False, seed=41, runs=2):
    """A captured PolicyRollout with a value head and GAE after `runs` runs: `kind` "gaussian" (continuous env, log_std = -0.5) or
    "categorical" (temperature TAU).  n a side, E games (env seed `seed`), the graph form (over `chains` game ranges) or one launch;
    opponent: None, or "red" / "blue" -- that team is played by the scripted instinct.Team and the actor learns the other;
    normalize: GAE's normalisation."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    A, D = 2 * n, 3 * n + 2
    cont = kind == "gaussian"
    torch.manual_seed(11)
    actor, critic = StackedActor(A, D, 3 if cont else 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(60.0); critic.w3.mul_(100.0)
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, continuous_actions=cont, device="cuda")
    env.reset()
    kw = {}
    if sample:
        kw = dict(sample="gaussian", log_std=torch.full((A, 3), -0.5, device="cuda")) if cont else dict(sample="categorical", temperature=TAU)
    if opponent is not None:
        mine, theirs = (env.possible_red, env.possible_blue) if opponent == "red" else (env.possible_blue, env.possible_red)
        kw["opponent"] = instinct.Team(mine, theirs, env)
    g = dict(gamma=0.99, lam=0.95, normalize=True) if normalize else dict(gamma=0.99, lam=0.95)
    ro = PolicyRollout(env, actor, T, seed=3, value_actor=critic, gae=g if gae else None, one_launch=one_launch, chains=chains, **kw)
    ro.start(); ro.capture()
    for _ in range(runs):
        ro.run()
    torch.cuda.synchronize()
    return ro


def scripted_columns(n, opponent):
    """(scripted, learned) agent columns of a rollout with opponent "red" / "blue" / None: a team's planes are adjacent columns, red first."""
    red, blue = list(range(n)), list(range(n, 2 * n))
    return {None: ([], red + blue), "red": (red, blue), "blue": (blue, red)}[opponent]


def nudge(net, scale, seed=5):
    """Every parameter moved by scale * mean|p| * a standard normal (drawn on the CPU: the same step on every device)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in PARAMS:
            p = getattr(net, k)
            p.add_((scale * p.abs().mean().cpu() * torch.randn(p.shape, generator=g)).to(p.device))
