"""The host restatement of the in-kernel Philox draws (tests/philox_util.py) checked on its own, with no GPU: the Random123
known-answer vectors for Philox4x32-10, and every code of uniforms4's 23-bit mapping."""
import numpy as np

import philox_util as pu


def _hex(words):
    return [f"{int(w):08x}" for w in words]


def test_philox4x32_10_known_answer_vectors():
    """Random123's kat_vectors for philox4x32_10: the restatement's rounds, multipliers and key schedule are the standard ones."""
    assert _hex(pu.philox4x32_10(0, 0, 0, 0, 0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    m = 0xFFFFFFFF
    assert _hex(pu.philox4x32_10(m, m, m, m, m, m)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _hex(pu.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_vectorised_philox_equals_the_scalar_calls():
    """A batch of counters gives, element by element, what one call per counter gives (no broadcasting mix-up)."""
    g = np.array([0, 1, 0xFFFFFFFF, 0x100000000, 0x123456789AB], np.uint64)
    batch = pu.actor_words(0x1_2345_6789, 77, g, pu.SALT_CATEGORICAL)
    for i, gi in enumerate(g):
        one = pu.actor_words(0x1_2345_6789, 77, np.array([gi], np.uint64), pu.SALT_CATEGORICAL)
        assert [int(w[i]) for w in batch] == [int(w[0]) for w in one]


def test_every_uniform_code_is_strictly_inside_the_unit_interval_and_increasing():
    """uniforms4's mapping (float(r >> 9) + 0.5f) * 2^-23 in float32, for all 2^23 codes: strictly inside (0, 1), strictly increasing,
    and exactly the odd multiples of 2^-24 (no code lost to rounding).  The 24-bit mapping it replaced failed all three at the top."""
    r = np.arange(1 << 23, dtype=np.uint32) << np.uint32(9)
    u = pu.uniform23(r)
    assert u.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert np.all(np.diff(u) > 0)
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, 2.0 * np.arange(1 << 23) + 1.0)
    # the low nine bits of the word do not move the value; the top word maps to the top code
    assert pu.uniform23(np.uint32(0xFFFFFFFF)) == u[-1] and pu.uniform23(np.uint32(0x1FF)) == u[0]
    # what the old 24-bit mapping did with the top code: float32 rounding to exactly 1.0
    assert (np.float32(0xFFFFFF) + np.float32(0.5)) * np.float32(2.0 ** -24) == np.float32(1.0)


def test_sampler_indices_stay_in_the_filled_rows():
    for M, counter in ((1, 5), (777, 776), (777, 10 ** 6), (999_983, 3)):
        idx = pu.sampler_indices(2 ** 33 + 5, 9, 4097, M, counter)
        assert idx.min() >= 0 and idx.max() < min(M, counter)
    assert not pu.sampler_indices(1, 2, 64, 777, 0).any() and not pu.sampler_indices(1, 2, 64, 777, -5).any()


def test_opponent_draws_are_in_range():
    d = pu.opponent_draws(2 ** 32 + 91, 3, np.arange(4096, dtype=np.uint64))
    assert d[:, 0].min() >= 0.0 and d[:, 0].max() < 1.0
    assert d[:, 1:].min() >= -0.15 and d[:, 1:].max() < 0.15
