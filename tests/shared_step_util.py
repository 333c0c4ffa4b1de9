"""What the tests of the tied optimiser step (learner.adam_step(group=), csrc/bsx_adam_step.hip: bsx_adam_step_shared) share:

  group_sum32            the float32 group gradient of the contract, on the host: the members' rows added in ascending agent order from
                         the leader's value on, one numpy float32 addition per member (each rounded on its own, never reassociated)
  leaders_rows           the gradient rows of the equivalent untied call: the group sum at every leader, +0 at every follower
  shared_reference_step  the contract in float64: the rows summed per group, adam_util.reference_step over the leaders only (a shared
                         parameter is ONE parameter: it counts once in the norm), the result broadcast to the members
"""
import numpy as np

import adam_util as U


def leaders(A, g):
    return list(range(0, A, g))


def group_sum32(row, g):
    """row: float32 array [A, ...] -> float32 [A // g, ...]: ((row[l] + row[l + 1]) + row[l + 2]) + ... per group, in float32."""
    row = np.ascontiguousarray(row, np.float32)
    A = row.shape[0]
    assert A % g == 0, (A, g)
    v = row.reshape(A // g, g, *row.shape[1:])
    acc = v[:, 0].copy()
    for k in range(1, g):
        acc = (acc + v[:, k]).astype(np.float32)
    assert acc.dtype == np.float32
    return acc


def leaders_rows(row, g):
    """row float32 [A, ...] -> float32 [A, ...]: group_sum32 at the leaders, +0 at the followers."""
    row = np.ascontiguousarray(row, np.float32)
    out = np.zeros_like(row)
    out[::g] = group_sum32(row, g)
    return out


def shared_reference_step(params, grads, m, v, t, hp, g):
    """One tied step in float64.  params, grads, m, v: lists of arrays with a leading agent axis A (the members of a group hold the same
    parameters and moments; the leaders' are the ones read); g: agents per group -> (params, m, v, t + 1, norm, coef) with the leading
    axis A again, every member holding its group's result."""
    A = params[0].shape[0]
    assert A % g == 0 and all(x.shape[0] == A for x in list(params) + list(grads) + list(m) + list(v))
    lead = lambda xs: [np.asarray(x, np.float64)[::g] for x in xs]     # noqa: E731
    gsum = [np.asarray(x, np.float64).reshape(A // g, g, *x.shape[1:]).sum(axis=1) for x in grads]
    P, M, V, t, norm, coef = U.reference_step(lead(params), gsum, lead(m), lead(v), t, hp)
    wide = lambda xs: [np.repeat(x, g, axis=0) for x in xs]            # noqa: E731
    return wide(P), wide(M), wide(V), t, norm, coef
