"""The float64 reference of the actor MLP (tests/actor_ref_util.py) pinned on the CPU, and the conditions the GPU comparisons of
tests/test_hip_actor_float64.py rest on, evaluated on the reference alone: a change of seed cannot make a GPU test quietly vacuous."""
import os

import numpy as np
import pytest
import torch

import actor_ref_util as au
from trace_util import GOLDEN


def test_head_sums64_reproduce_the_recorded_outputs_of_the_shipped_checkpoints():
    """Fixture g12: the unmodified reference network's outputs on rows met in its own play.  2e-5 after tanh, the fixture's own bar
    (the recording is float32 in another summation order)."""
    from deep_rl_battlespace_amd.rollout import reference_checkpoint_actor
    z = np.load(os.path.join(GOLDEN, "g12_evaluation.npz"))
    n = int(z["n_agents"])
    actor = reference_checkpoint_actor(z, n, device="cpu")
    x = torch.stack([torch.from_numpy(z[f"plane{i % n}/x"]) for i in range(2 * n)], 1)
    y = au.head_sums64(actor, x)
    assert y.dtype == np.float64 and y.shape == (96, 2 * n, 4)
    for i in range(2 * n):
        err = np.abs(np.tanh(y[:, i]) - z[f"plane{i % n}/y"].astype(np.float64))
        print(f"plane {i}: max |tanh(y64) - recorded| = {err.max():.2e}")
        assert err.max() <= 2e-5
    # the float32 yardstick is the same network: it differs from the float64 sums by rounding only
    assert np.abs(au.head_sums32(actor, x) - y).max() < 1e-4 * max(1.0, np.abs(y).max())


@pytest.mark.parametrize("n", [1, 2])
def test_split_model_is_the_emulated_bf16_path(n):
    """split_model64 and the lane-by-lane MFMA emulation are both float64 arithmetic on the same bfloat16 terms -- one reads the
    weights from the module, the other from the packed blob through the kernel's index maps: 1e-9 on the head sums, or one of the
    two misreads the blob.  The emulation's float32 path against head_sums64 likewise."""
    actor, obs = au.fresh(n, seed=n, outputs=4)
    obs = obs[:64].contiguous()
    em = au.mfma_emulation(actor, obs)
    y64 = au.head_sums64(actor, obs)
    m2, m3 = au.split_model64(actor, obs, 2), au.split_model64(actor, obs, 3)
    for a in range(2 * n):
        d2 = np.abs(em[a]["sums"]["bf16x3"] - m2[:, a]).max()
        d3 = np.abs(em[a]["sums"]["bf16x6"] - m3[:, a]).max()
        d0 = np.abs(em[a]["sums"]["f32"] - y64[:, a]).max()
        print(f"n={n} agent {a}: emulation - model: two terms {d2:.1e}, three terms {d3:.1e}; f32 path - float64 {d0:.1e}")
        assert d2 <= 1e-9 and d3 <= 1e-9 and d0 <= 1e-9
    # and the split does lose what it is said to lose: two terms ~2^-16 relative on the layer, three terms float32-class
    e2, e3 = np.abs(m2 - y64).max(), np.abs(m3 - y64).max()
    assert 1e-7 < e2 < 1e-4 and e3 < e2 / 50


def test_as_critics_pack_the_policy_with_the_other_head_columns_zeroed():
    for n, outputs in ((2, 4), (3, 3)):
        actor, obs = au.trained_like(n, outputs=outputs)
        crit = au.as_critics(actor)
        assert len(crit) == outputs
        y = au.head_sums64(actor, obs[:50])
        for k, c in enumerate(crit):
            assert c.n_actions == 1
            other = au.to_cpu32(actor)
            with torch.no_grad():
                w3, b3 = torch.zeros_like(other.w3), torch.zeros_like(other.b3)
                w3[:, :, 0] = actor.w3[:, :, k]; b3[:, :, 0] = actor.b3[:, :, k]
                other.w3.copy_(w3); other.b3.copy_(b3)
            assert torch.equal(c.pack(), other.pack()), k
            assert np.array_equal(au.head_sums64(c, obs[:50])[..., 0], y[..., k])


@pytest.mark.parametrize("cls,n", au.COMBOS)
def test_conditions_of_the_gpu_comparisons_hold_on_the_reference(cls, n):
    """Every class at its test size has at least 1 000 outputs with |y64| < 1 -- where the score check sees the body's error --, the
    yardsticks are ordered as the bounds assume (two terms lose far more than float32, three terms do not), and each class is what its
    name says."""
    actor, obs = au.CLASSES[cls](n)
    actor.requires_grad_(False)
    y, e_t, e_m2, e_m3 = au.reference_errors(cls, n)
    E, A, D = au.dense_games(n), 2 * n, 3 * n + 2
    assert tuple(obs.shape) == (E, A, D) and y.shape == (E, A, actor.n_actions) and E % 64 != 0
    assert np.isfinite(y).all()
    small = int((np.abs(y) < 1).sum())
    print(f"{cls} n={n}: {y.size} outputs, {small} with |y64| < 1, max |y64| {np.abs(y).max():.1f}; e_t {e_t.max():.2e} / {e_t.mean():.2e}, "
          f"e_m2 {e_m2.max():.2e} / {e_m2.mean():.2e}, e_m3 {e_m3.max():.2e} / {e_m3.mean():.2e}")
    assert small >= 1000
    assert e_m2.mean() > 8 * e_t.mean() and e_m3.mean() < e_t.mean()
    if cls == "shipped":
        assert float(actor.w2.abs().max()) > 10 and float(max(actor.g1.abs().max(), actor.g2.abs().max())) > 4.9
        assert np.abs(y).max() > 50 and (np.abs(y) > 4).mean() > 0.6
    if cls == "trained_like":
        for g in (actor.g1, actor.g2):
            assert bool((g < 0).any()) and bool((g.abs() < 0.1).any()) and float(g.abs().max()) > 4
        assert float(actor.w2.abs().max()) > 0.9
    if cls == "flat_rows":
        with torch.no_grad():
            a64 = au.to_float64(actor)
            var = torch.baddbmm(a64.b1, obs.double().transpose(0, 1), a64.w1).var(-1, unbiased=False)
        assert float(var.max()) < 1e-5 / 100                  # rsqrt(var + eps) is rsqrt(eps) to 1 %
    if cls == "dead_half":
        assert bool((obs[::2] == -1).all()) and not bool((obs[1::2] == -1).all())
    if cls == "wide_obs":
        assert float(obs.abs().max()) > 7.9
        for e, v in zip(au.TILE_EDGES, au.EDGE_VALUES):
            assert bool((obs[e] == v).all())


@pytest.mark.parametrize("layer", [1, 2])
def test_every_localisation_case_has_its_neuron_active_on_a_quarter_of_the_rows(layer):
    """... and the output depends on the input through that neuron alone: with the neuron's row of W2 / W3 zeroed as well, the
    float64 output is the same on every row."""
    seen = []
    for launch in range(8):
        actor, obs, neurons, active = au.localisation_case(layer, launch)
        seen += neurons
        assert min(active) >= 0.25, (launch, active)
        assert max(active) <= 0.75, (launch, active)           # (and silent on a quarter: the ReLU's kink is in play)
        w = actor.w2 if layer == 1 else actor.w3
        assert int((w != 0).any(-1).sum()) == len(neurons)      # one non-zero row per agent
        assert bool((actor.b1 != 0).all()) and bool((actor.b2 != 0).all()) and bool((actor.b3 != 0).all())
        assert np.abs(au.head_sums64(actor, obs)).max() < 2     # tanh hides nothing: the rollout form of the test sees scores only
        y = au.head_sums64(actor, obs[:64])
        assert (y.max(0) - y.min(0)).min() > 1e-3               # the outputs do move with the input
        with torch.no_grad():
            w.zero_()
        y0 = au.head_sums64(actor, obs[:64])
        assert np.abs(y0 - y0[:1]).max() == 0
    assert sorted(seen) == list(range(64))
