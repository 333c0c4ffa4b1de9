"""GAE(gamma, lambda) advantages and returns on device, for on-policy learners (csrc/bsx_advantage.hip, `bsx_gae`).

    adv, ret, mask, stats = gae(ro.rew, ro.value, last_value, ro.done, ro.env_done, done_prev, 0.99, 0.95)

The inputs are a rollout's records in PolicyRollout's layout (tick-major, contiguous): `rew`, `value` f32 [T, E, A], `done`
[T, E, A] (the agent's flag after tick t), `env_done` [T(+1), E] (the game's flag before tick t), `last_value` f32 [E, A] = V(obs[T])
and `done_prev` [E, A], the agent's flag before tick 0 -- a carry that the call sets to done[T-1].  A row counts (`mask`) when its game
was running and its agent alive before the tick: rows after an agent's death, inert ticks and auto-reset re-spawn rows get adv = ret = 0,
and rewards on them are dropped.  Death, a win or loss and the time-limit tie are terminal and never bootstrapped.  The exact contract
(float32 operations each rounded on their own) is written out in include/battlespace_hip.h next to `bsx_gae`.

One launch on the current stream, with no host synchronisation, so it can be captured into a graph (PolicyRollout(gae=...) does).
normalize=True adds a masked float64 mean / unbiased std of the advantages (two more launches, fixed merge order: the same bits on every
call) into `stats` = (n, mean, std) and scales the masked advantages by them; `ret` stays as it is.  Works on any tensors of these shapes,
e.g. a continuous-action rollout whose values come from the caller's own torch critic.

agents= (bool / uint8 [A] on the device; `bsx_gae_agents`): the agents the actor plays.  One whose flag is 0 -- a scripted opponent's plane --
has no decisions: mask 0 and adv = ret = +0 on all of its rows, which are in none of the statistics; its carry in `done_prev` is still
updated.  PolicyRollout(opponent=..., gae=...) passes the learned team's flags.
"""
from collections import namedtuple
from functools import partial

import torch

from . import _lib
from ._args import _F32, _FLAG, _need, _workspace

Gae = namedtuple("Gae", "adv ret mask stats")


def check_rates(gamma, lam):
    """gamma, lam: floats in [0, 1] (NaN refused); the kernel takes them as float32."""
    for name, x in (("gamma", gamma), ("lam", lam)):
        try:
            ok = 0.0 <= float(x) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{name} must be a number in [0, 1], got {x!r}")


def workspace_bytes(E, A, T):
    """Bytes of the workspace that gae(..., normalize=True) needs for E games of A agents and T ticks."""
    return _lib.query_bytes("bsx_gae_workspace_bytes", E, A, T)


def gae(rew, value, last_value, done, env_done, done_prev, gamma, lam, *, normalize=False, out=None, stats=None, workspace=None, agents=None):
    """-> Gae(adv f32 [T, E, A], ret f32 [T, E, A], mask bool [T, E, A], stats f64 [3] or None); done_prev is updated in place.
    agents: optional bool / uint8 [A] device tensor, 0 = an agent the actor does not play (no decisions: see the module's docstring).
    out: optional (adv, ret, mask) to write into (mask uint8 or bool).  stats (f64 [3]) and workspace (uint8, at least
    workspace_bytes(E, A, T)) are allocated when normalize=True and they are not given -- pass them for a captured graph."""
    if not isinstance(rew, torch.Tensor) or rew.dim() != 3:
        raise ValueError("rew must be a float32 [T, E, A] tensor")
    T, E, A = rew.shape
    dev = rew.device
    if dev.type != "cuda":
        raise ValueError("gae runs on the GPU: rew is on " + str(dev))
    if T < 1 or E < 1 or A < 2 or A % 2:
        raise ValueError(f"rew has shape {tuple(rew.shape)}: T >= 1, E >= 1 and an even A >= 2 are needed")
    check_rates(gamma, lam)
    need = partial(_need, dev=dev, anchor="rew")
    need(rew, "rew", (T, E, A), _F32)
    need(value, "value", (T, E, A), _F32)
    need(last_value, "last_value", (E, A), _F32)
    need(done, "done", (T, E, A), _FLAG)
    if not isinstance(env_done, torch.Tensor) or env_done.dim() != 2 or env_done.shape[0] < T:
        raise ValueError(f"env_done must be a [T(+1), E] tensor with at least {T} rows")
    need(env_done, "env_done", (env_done.shape[0], E), _FLAG)
    need(done_prev, "done_prev", (E, A), _FLAG)
    if agents is not None:
        need(agents, "agents", (A,), _FLAG)
    if out is None:
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        mask = torch.empty((T, E, A), dtype=torch.uint8, device=dev)
    else:
        adv, ret, mask = out
        need(adv, "out adv", (T, E, A), _F32)
        need(ret, "out ret", (T, E, A), _F32)
        need(mask, "out mask", (T, E, A), _FLAG)
    if normalize:
        if stats is None:
            stats = torch.zeros(3, dtype=torch.float64, device=dev)
        need(stats, "stats", (3,), (torch.float64,))
        workspace = _workspace(workspace, workspace_bytes(E, A, T), dev)
    io = _lib.BsxGaeIo(rew.data_ptr(), value.data_ptr(), done.data_ptr(), env_done.data_ptr(), last_value.data_ptr(), done_prev.data_ptr(),
                       adv.data_ptr(), ret.data_ptr(), mask.data_ptr())
    lib = _lib.load()
    _lib.check(lib.bsx_gae_agents(_lib.ctypes.byref(io), agents.data_ptr() if agents is not None else None, int(T), int(E), int(A), float(gamma),
                                  float(lam), 1 if normalize else 0, workspace.data_ptr() if normalize else None,
                                  stats.data_ptr() if normalize else None, torch.cuda.current_stream(dev).cuda_stream), "bsx_gae_agents")
    return Gae(adv, ret, mask.view(torch.bool) if mask.dtype == torch.uint8 else mask, stats if normalize else None)
