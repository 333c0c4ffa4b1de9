"""CPU-side checks of the Gaussian policy head (bsx_actor_forward_gaussian, bsx_rollout_continuous_gaussian, PolicyRollout(sample="gaussian")):
the header and the binding agree on the struct and the entry points; every refusal of the new entry points comes before any launch, in a
pinned order (fake addresses only: no call here reaches a kernel); the existing entry points keep their refusals; PolicyRollout validates
its arguments on a stub env; the learner-side log-probability matches torch.distributions."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN = -1, -2
P, M = 4096, 4096 + 8          # a 256-byte aligned fake address and one aligned to 8 bytes only (neither is dereferenced)


def _lib():
    from deep_rl_battlespace_amd import _lib as L
    return L


def _header():
    return open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()


def test_header_and_binding_agree_on_the_gaussian_head():
    L = _lib()
    hdr = _header()
    body = re.search(r"typedef struct BsxGaussianHead \{(.*?)\} BsxGaussianHead;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f for f, _ in L.BsxGaussianHead._fields_] == ["log_std", "logp"]
    assert ctypes.sizeof(L.BsxGaussianHead) == 16
    for name in ("bsx_actor_forward_gaussian", "bsx_rollout_continuous_gaussian"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert name in L.SIGNATURES
        assert hasattr(L.load(), name)
    # the head comes right after the noise struct, and everything else is the plain entry point's argument list
    for plain, gauss in (("bsx_actor_forward", "bsx_actor_forward_gaussian"), ("bsx_rollout_continuous", "bsx_rollout_continuous_gaussian")):
        a, b = L.SIGNATURES[plain][1], L.SIGNATURES[gauss][1]
        i = a.index(ctypes.POINTER(L.BsxActorNoise))
        assert b[:i + 1] == a[:i + 1] and b[i + 1] == ctypes.POINTER(L.BsxGaussianHead) and b[i + 2:] == a[i + 1:]
    assert re.search(r"#define BSX_ABI_VERSION (\d+)", hdr).group(1) == "14" and L.load().bsx_abi_version() == 14
    src = open(os.path.join(ROOT, "deep-rl-battlespace_amd", "csrc", "bsx_actor_core.h")).read()
    assert re.search(r"GAUSS_SALT = 0xC0000000u", src)


def _noise(L, **fields):
    nz = L.BsxActorNoise()
    for k, v in fields.items():
        setattr(nz, k, v)
    return ctypes.byref(nz)


def _head(L, log_std=P, logp=None):
    return ctypes.byref(L.BsxGaussianHead(log_std, logp))


def test_actor_forward_gaussian_refuses_before_any_launch():
    L = _lib(); lib = L.load()

    def fwd(w=P, obs=P, scores=P, E=4, n=1, prec=0, nz=None, head="ok", off=0):
        h = _head(L) if head == "ok" else head
        return lib.bsx_actor_forward_gaussian(w, obs, scores, E, n, prec, nz, h, 0, 0, None, off, None)

    cases = [(ARG, dict(head=None)), (ARG, dict(head=_head(L, log_std=None))), (ARG, dict(obs=None)), (ARG, dict(scores=None)),
             (ARG, dict(prec=3)), (ARG, dict(w=None)), (ARG, dict(E=0)), (ARG, dict(n=0)), (ARG, dict(n=17)), (ARG, dict(off=-1)),
             (ARG, dict(nz=_noise(L, gaussian_std=0.1))), (ARG, dict(nz=_noise(L, ou_scale=0.5, ou_state=P))),
             (ARG, dict(nz=_noise(L, sample_mode=1, temperature=1.0))), (ARG, dict(nz=_noise(L, sample_mode=2, temperature=1.0))),
             (ARG, dict(nz=_noise(L, u_inject=P))), (ARG, dict(nz=_noise(L, logp=P))), (ARG, dict(nz=_noise(L, value_weights=P))),
             (ALIGN, dict(w=M + 4)), (ALIGN, dict(scores=M)), (ALIGN, dict(obs=P + 2)), (ALIGN, dict(head=_head(L, log_std=P + 2))),
             (ALIGN, dict(head=_head(L, logp=P + 2))), (ALIGN, dict(nz=_noise(L, z_inject=M))),
             (ALIGN, dict(nz=_noise(L, value_weights=M, value=P))), (ALIGN, dict(nz=_noise(L, value_weights=P, value=P + 2)))]
    # two rules broken at once: which check comes first is part of the contract
    cases += [(ARG, dict(head=None, scores=M)), (ARG, dict(head=None, w=None)), (ARG, dict(head=_head(L, log_std=None), obs=P + 2)),
              (ARG, dict(obs=None, head=None)), (ALIGN, dict(scores=M, nz=_noise(L, gaussian_std=0.1))),
              (ALIGN, dict(w=M + 4, head=_head(L, log_std=P + 2))), (ARG, dict(nz=_noise(L, gaussian_std=0.1), head=_head(L, log_std=P + 2))),
              (ARG, dict(nz=_noise(L, logp=P + 2))), (ALIGN, dict(head=_head(L, log_std=P + 2), nz=_noise(L, z_inject=M))),
              (ALIGN, dict(head=_head(L, logp=P + 2), nz=_noise(L, value_weights=P))), (ARG, dict(off=-1, nz=_noise(L, z_inject=P)))]
    for want, kw in cases:
        assert fwd(**kw) == want, kw


def test_rollout_continuous_gaussian_refuses_before_any_launch():
    L = _lib(); lib = L.load()
    rw = ctypes.byref(L.BsxRewards(100, 10, -1, -5, -20))

    def ro(state=P, E=4, n=1, T=8, w=P, prec=0, team=-1, obs=P, scores=P, rew=P, done=P, cfg=rw, flags=0, nz=None, head="ok"):
        h = _head(L) if head == "ok" else head
        return lib.bsx_rollout_continuous_gaussian(state, E, n, T, w, prec, team, 0, obs, scores, rew, done, None, None, None, cfg, flags,
                                                   nz, h, 0, 0, None, 0, 0, None)

    cases = [(ARG, dict(head=None)), (ARG, dict(head=_head(L, log_std=None))), (ARG, dict(state=None)), (ARG, dict(E=0)),
             (ARG, dict(n=5)), (ARG, dict(T=0)), (ARG, dict(T=65536)), (ARG, dict(w=None)), (ARG, dict(obs=None)), (ARG, dict(scores=None)),
             (ARG, dict(rew=None)), (ARG, dict(done=None)), (ARG, dict(cfg=None)), (ARG, dict(flags=2)), (ARG, dict(prec=3)),
             (ARG, dict(team=2)), (ARG, dict(nz=_noise(L, gaussian_std=0.1))), (ARG, dict(nz=_noise(L, ou_scale=0.5, ou_state=P))),
             (ARG, dict(nz=_noise(L, sample_mode=1, temperature=1.0))), (ARG, dict(nz=_noise(L, sample_mode=2, temperature=1.0))),
             (ARG, dict(nz=_noise(L, u_inject=P))), (ARG, dict(nz=_noise(L, logp=P))), (ARG, dict(nz=_noise(L, z_inject=P))),
             (ARG, dict(n=2, nz=_noise(L, value_weights=P, value=P))), (ARG, dict(nz=_noise(L, value_weights=P))),
             (ALIGN, dict(state=M)), (ALIGN, dict(w=M)), (ALIGN, dict(scores=M)), (ALIGN, dict(obs=P + 2)), (ALIGN, dict(rew=P + 2)),
             (ALIGN, dict(head=_head(L, log_std=P + 2))), (ALIGN, dict(head=_head(L, logp=P + 2))),
             (ALIGN, dict(nz=_noise(L, value_weights=M, value=P)))]
    cases += [(ARG, dict(head=None, state=M)), (ARG, dict(head=None, T=0)), (ARG, dict(T=0, head=_head(L, log_std=P + 2))),
              (ALIGN, dict(state=M, nz=_noise(L, gaussian_std=0.1))), (ALIGN, dict(scores=M, head=_head(L, log_std=P + 2))),
              (ARG, dict(nz=_noise(L, sample_mode=1, temperature=1.0), head=_head(L, logp=P + 2))),
              (ALIGN, dict(head=_head(L, logp=P + 2), nz=_noise(L, z_inject=P))),
              (ALIGN, dict(head=_head(L, log_std=P + 2), nz=_noise(L, value_weights=P, value=P, ou_state=M)))]
    for want, kw in cases:
        assert ro(**kw) == want, kw


def test_existing_entry_points_keep_their_refusals():
    L = _lib(); lib = L.load()
    rw = ctypes.byref(L.BsxRewards(100, 10, -1, -5, -20))

    def cont(nz):
        return lib.bsx_rollout_continuous(P, 4, 1, 8, P, 0, -1, 0, P, P, P, P, None, None, None, rw, 0, nz, 0, 0, None, 0, 0, None)
    assert cont(_noise(L, sample_mode=1, temperature=1.0)) == ARG                   # a categorical head on continuous actions
    assert cont(_noise(L, sample_mode=2, temperature=1.0)) == ARG
    assert cont(_noise(L, z_inject=P)) == ARG
    assert lib.bsx_rollout_discrete(P, 4, 2, 8, P, 0, -1, P, P, P, P, None, None, None, rw, 0, _noise(L, value_weights=P, value=P),
                                    0, 0, None, 0, 0, None) == ARG                  # a value head in the discrete one-launch kernel at n = 2
    assert lib.bsx_actor_forward(P, P, P, 4, 1, 0, _noise(L, sample_mode=2, temperature=1.0), 0, 0, None, 0, None) == ARG
    assert lib.bsx_actor_forward(P, P, M, 4, 1, 0, None, 0, 0, None, 0, None) == ALIGN


def _stub_env(n=1, E=8, continuous=True):
    return types.SimpleNamespace(_compat=False, rng="philox", continuous_actions=continuous, n_agents=n, n_envs=E, _A=2 * n,
                                 obs_size=3 * n + 2, device=torch.device("cpu"), env_offset=0)


def test_policy_rollout_validates_the_gaussian_head():
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    env, actor, critic = _stub_env(), StackedActor(2, 5, 3), StackedActor(2, 5, 1)
    ls = torch.zeros((2, 3))
    with pytest.raises(ValueError, match="continuous"):
        PolicyRollout(_stub_env(continuous=False), StackedActor(2, 5, 4), 4, sample="gaussian", log_std=ls, chains=1)
    for bad in (None, torch.zeros((2, 4)), torch.zeros((3, 3)), torch.zeros((2, 3), dtype=torch.float64), torch.zeros((3, 2)).t(), ls.numpy()):
        with pytest.raises(ValueError, match="log_std"):
            PolicyRollout(env, actor, 4, sample="gaussian", log_std=bad, chains=1)
    with pytest.raises(ValueError, match="exploration noise"):
        PolicyRollout(env, actor, 4, sample="gaussian", log_std=ls, noise_std=0.1, chains=1)
    with pytest.raises(ValueError, match="exploration noise"):
        PolicyRollout(env, actor, 4, sample="gaussian", log_std=ls, ou_scale=0.2, chains=1)
    with pytest.raises(ValueError, match="fused"):
        PolicyRollout(env, actor, 4, sample="gaussian", log_std=ls, fused=False, chains=1)
    with pytest.raises(ValueError, match="log_std"):
        PolicyRollout(env, actor, 4, log_std=ls, chains=1)                        # a log-std without the head
    with pytest.raises(ValueError, match="categorical"):
        PolicyRollout(env, actor, 4, sample="categorical", chains=1)              # still refused on a continuous env
    with pytest.raises(ValueError, match="3 for a continuous"):
        PolicyRollout(env, StackedActor(2, 5, 4), 4, sample="gaussian", log_std=ls, chains=1)
    ro = PolicyRollout(env, actor, 4, sample="gaussian", log_std=ls, value_actor=critic, gae=dict(gamma=0.99, lam=0.95), chains=1)
    assert ro.log_std is ls and tuple(ro.logp.shape) == (4, 8, 2) and tuple(ro.value.shape) == (4, 8, 2) and tuple(ro.adv.shape) == (4, 8, 2)
    ro = PolicyRollout(env, actor, 4, value_actor=critic, gae=dict(gamma=0.99, lam=0.95), chains=1)   # a value head on a continuous env
    assert ro.logp is None and ro.value is not None
    ro = PolicyRollout(env, actor, 4, sample="gaussian", log_std=ls, value_actor=critic, one_launch=True)
    assert ro.one_launch
    with pytest.raises(ValueError, match="1v1"):
        PolicyRollout(_stub_env(n=2), StackedActor(4, 8, 3), 4, sample="gaussian", log_std=torch.zeros((4, 3)),
                      value_actor=StackedActor(4, 8, 1), one_launch=True)


def test_fused_actor_head_struct_validates():
    from deep_rl_battlespace_amd.rollout import FusedActor, StackedActor
    fa = FusedActor(StackedActor(2, 5, 3), 1)
    ls, lp = torch.zeros((2, 3)), torch.zeros((6, 2))
    h = fa.head_struct(6, dict(log_std=ls, logp=lp))
    assert h.log_std == ls.data_ptr() and h.logp == lp.data_ptr()
    assert fa.head_struct(6, dict(log_std=ls)).logp is None
    for bad in (dict(log_std=torch.zeros((2, 4))), dict(log_std=ls, logp=torch.zeros((5, 2))), dict(log_std=ls, logp=torch.zeros((6, 2), dtype=torch.float64))):
        with pytest.raises(ValueError):
            fa.head_struct(6, bad)
    with pytest.raises(ValueError, match="exploration noise"):
        fa.head_struct(6, dict(log_std=ls), noise_std=0.1)
    with pytest.raises(ValueError, match="3 outputs"):
        FusedActor(StackedActor(2, 5, 4), 1).head_struct(6, dict(log_std=ls))


def test_gaussian_log_prob_is_the_diagonal_normal():
    from deep_rl_battlespace_amd.rollout import StackedActor, gaussian_log_prob
    torch.manual_seed(0)
    actor = StackedActor(4, 8, 3)
    obs, ls = torch.randn(3, 5, 4, 8), 0.3 * torch.randn(4, 3)
    act = torch.cat([2.0 * torch.randn(3, 5, 4, 3), torch.full((3, 5, 4, 1), 7.0)], -1)      # |a| > 1 occurs; column 3 is ignored
    logp, ent = gaussian_log_prob(actor, ls, obs, act)
    with torch.no_grad():
        mu = torch.stack([actor(o) for o in obs])
    dist = torch.distributions.Normal(mu, torch.exp(ls))
    torch.testing.assert_close(logp, dist.log_prob(act[..., :3]).sum(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ent, dist.entropy().sum(-1), rtol=1e-6, atol=1e-6)
    z = (act[..., :3] - mu) / torch.exp(ls)
    torch.testing.assert_close(logp, (-0.5 * z * z - ls).sum(-1) - 1.5 * math.log(2 * math.pi), rtol=1e-5, atol=1e-5)
    ls.requires_grad_(True)
    gaussian_log_prob(actor, ls, obs, act)[0].sum().backward()
    assert ls.grad is not None and actor.w1.grad is not None
