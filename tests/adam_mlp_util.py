"""The host side of what the tests of the free-width optimiser step with Polyak targets (learner.mlp_adam_step, bsx_adam_step_mlp)
share, on top of tests/adam_util.py (the cases on the GPU and the torch yardstick are tests/adam_case_util.py's):

  SHAPES             the (A, D, n_actions) of the issue: the smallest, an odd A at the 1v1 critic's width, the 2v2 critic, the first width
                     beyond the old LDS bound (odd D, pad columns), the widest row (8 full strides of 1024 and a ragged ninth) and the
                     widest call (32 agents x 2 networks + log_std = 65 partials)
  blob_floats        floats per agent of StackedActor.pack() at any width
  polyak             the contract's Polyak line restated in float64: t = (1 - tau) t + tau p, tau the float32 value the device reads
  reference_step     adam_util.reference_step followed by polyak on the networks that have a target
"""
import numpy as np

import adam_util as U

#          id             A   D  n_actions  second network (1 column) and log_std
SHAPES = {"a1-d1": (1, 1, 1, False), "a3-d9": (3, 9, 1, False), "a4-d24": (4, 24, 1, False), "a5-d51-na3": (5, 51, 3, False),
          "a2-d64-na4": (2, 64, 4, False), "a32-d64-two-nets-log-std": (32, 64, 1, True)}
TAU = float(np.float32(0.01))


def blob_floats(D):
    """Floats per agent of StackedActor.pack() at any width: W1A over D rounded up to even, and 10 884 more."""
    return 64 * (D + D % 2) + 10884


def polyak(targets, params, tau):
    """t = (1 - tau) t + tau p in float64 over two lists of arrays -> new arrays.  tau: a float32-representable Python float."""
    return [(1.0 - tau) * np.asarray(t, np.float64) + tau * np.asarray(p, np.float64) for t, p in zip(targets, params)]


def reference_step(params, grads, m, v, targets, t, hp, tau):
    """adam_util.reference_step over everything in the call, then the Polyak line.  targets: a list as long as params with None where
    a tensor has no target (a network without one, log_std) -> (params, m, v, targets, t + 1, norm, coef)."""
    P, M, V, t, norm, coef = U.reference_step(params, grads, m, v, t, hp)
    T = [None if x is None else polyak([x], [p], tau)[0] for x, p in zip(targets, P)]
    return P, M, V, T, t, norm, coef
