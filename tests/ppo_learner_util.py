"""The small rollout the PPO learner's GPU tests share (the record of tests/test_hip_actor_grad.py's PPO test: n = 1, E = 96, T = 8,
head weights scaled to trained size), built fresh for each caller: the tests move its networks."""
import torch

PARAMS = ("w1", "b1", "g1", "h1", "w2", "b2", "g2", "h2", "w3", "b3")
TAU = 0.7


def small_rollout(kind, gae=True, sample=True, T=8):
    """A captured PolicyRollout with a value head and GAE after two runs: `kind` "gaussian" (continuous env, log_std = -0.5) or
    "categorical" (temperature TAU)."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    n, E = 1, 96
    A, D = 2 * n, 3 * n + 2
    cont = kind == "gaussian"
    torch.manual_seed(11)
    actor, critic = StackedActor(A, D, 3 if cont else 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(60.0); critic.w3.mul_(100.0)
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=41, auto_reset=True, continuous_actions=cont, device="cuda")
    env.reset()
    kw = {}
    if sample:
        kw = dict(sample="gaussian", log_std=torch.full((A, 3), -0.5, device="cuda")) if cont else dict(sample="categorical", temperature=TAU)
    ro = PolicyRollout(env, actor, T, seed=3, value_actor=critic, gae=dict(gamma=0.99, lam=0.95) if gae else None, **kw)
    ro.start(); ro.capture()
    ro.run(); ro.run()
    torch.cuda.synchronize()
    return ro


def nudge(net, scale, seed=5):
    """Every parameter moved by scale * mean|p| * a standard normal (drawn on the CPU: the same step on every device)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in PARAMS:
            p = getattr(net, k)
            p.add_((scale * p.abs().mean().cpu() * torch.randn(p.shape, generator=g)).to(p.device))
