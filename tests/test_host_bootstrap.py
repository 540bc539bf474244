"""The counter-based shuffle generator of the device bootstrap (pyaudiolocalization_amd/bootstrap.py), on the host: every mode
is a bijection, block and circular mode keep the reference's meaning (utils.py:196-205), the key separates seed / i / j / s,
and the output position of every input index is uniform."""
import numpy as np
import pytest

from pyaudiolocalization_amd import bootstrap as B

MODES = ("permutation", "block", "circular")
LENGTHS = (1, 2, 3, 7, 64, 1000, 2026, 44100, 88199)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_shuffle_is_a_bijection(L, mode):
    for s in (0, 1, 999):
        idx = B.shuffle_indices(L, 3, 11, s, mode, block_size=50, seed=5)
        assert idx.dtype == np.int64 and idx.shape == (L,)
        assert np.array_equal(np.sort(idx), np.arange(L))


def test_block_mode_moves_whole_blocks():
    L, bs = 2026, 50                                   # 41 blocks, the last one 26 samples long
    row = np.arange(L, dtype=np.float64)
    blocks = [row[k * bs:(k + 1) * bs] for k in range(-(-L // bs))]
    seen_short_at = set()
    for s in range(20):
        out = row[B.shuffle_indices(L, 0, 1, s, "block", block_size=bs, seed=2)]
        pos, order = 0, []
        while pos < L:                                 # walk the output block by block: each piece is one whole source block
            k = int(out[pos]) // bs
            blk = blocks[k]
            assert np.array_equal(out[pos:pos + len(blk)], blk), (s, pos, k)
            if len(blk) < bs:
                seen_short_at.add(pos)
            order.append(k)
            pos += len(blk)
        assert sorted(order) == list(range(len(blocks)))
        # the reference's construction with this block order
        assert np.array_equal(out, np.concatenate([blocks[k] for k in order])[:L])
    assert len(seen_short_at) > 1                      # the short block lands in different places


def test_block_size_at_least_the_row_is_the_identity():
    assert np.array_equal(B.shuffle_indices(37, 1, 2, 3, "block", block_size=37), np.arange(37))
    assert np.array_equal(B.shuffle_indices(37, 1, 2, 3, "block", block_size=1000), np.arange(37))


def test_circular_mode_is_a_roll():
    row = np.random.default_rng(1).standard_normal(1001)
    shifts = set()
    for s in range(50):
        key = B.shuffle_key(9, 4, 7, s)
        shift = B.circular_shift(key, row.size)
        assert 0 <= shift < row.size
        assert np.array_equal(row[B.shuffle_indices(row.size, 4, 7, s, "circular", seed=9)], np.roll(row, shift))
        shifts.add(shift)
    assert len(shifts) > 40


@pytest.mark.parametrize("mode", MODES)
def test_key_determinism_and_separation(mode):
    L, base = 2026, dict(i=2, j=5, s=17, seed=123)

    def draw(**kw):
        a = dict(base, **kw)
        return B.shuffle_indices(L, a["i"], a["j"], a["s"], mode, block_size=50, seed=a["seed"])

    ref = draw()
    assert np.array_equal(ref, draw())
    for change in (dict(seed=124), dict(i=3), dict(j=6), dict(s=18), dict(i=5, j=2)):
        assert not np.array_equal(ref, draw(**change)), change


def _chi2_limit(dof):
    # chi-square quantile at alpha = 1e-3 (Wilson-Hilferty; scipy's isf(1e-3, 36) = 67.985)
    z = 3.090232306167813
    return dof * (1 - 2 / (9 * dof) + z * np.sqrt(2 / (9 * dof))) ** 3


def test_uniform_positions_and_shifts():
    L, n = 37, 20000
    counts = np.zeros((L, L))                          # counts[input index, output position]
    shift_counts = np.zeros(L)
    for k in range(n):
        i, j, s = k % 5, 5 + k // 5 % 11, k
        idx = B.shuffle_indices(L, i, j, s, "permutation", seed=77)
        counts[idx, np.arange(L)] += 1
        shift_counts[B.circular_shift(B.shuffle_key(77, i, j, s), L)] += 1
    expect = n / L
    limit = _chi2_limit(L - 1)
    assert abs(limit - 67.985) < 0.2
    stats = ((counts - expect) ** 2 / expect).sum(axis=1)
    assert stats.max() < limit, stats.max()
    assert ((shift_counts - expect) ** 2 / expect).sum() < limit


def test_argument_checks():
    with pytest.raises(ValueError):
        B.shuffle_indices(10, 0, 1, 0, "shuffle")
    with pytest.raises(ValueError):
        B.shuffle_indices(10, 0, 1, 0, "block", block_size=0)
    with pytest.raises(ValueError):
        B.check_args("permutation", 50, num_bootstrap=0)
    with pytest.raises(ValueError):
        B.check_args(3, 50)
    assert [B.check_args(m, 1) for m in MODES] == [0, 1, 2]


def test_device_entry_points_check_arguments_before_the_engine():
    """utils.bootstrap_thresholds refuses bad arguments before it touches the engine (no GPU needed to see the error)."""
    from pyaudiolocalization_amd import utils as U
    rows, pairs = np.zeros((2, 16)), [[0, 1]]
    with pytest.raises(ValueError):
        U.bootstrap_thresholds(rows, pairs, 16000.0, bootstrap_mode="nope")
    with pytest.raises(ValueError):
        U.bootstrap_thresholds(rows, pairs, 16000.0, block_size=0)
    with pytest.raises(ValueError):
        U.bootstrap_thresholds(rows, pairs, 16000.0, num_bootstrap=0)
    with pytest.raises(ValueError):
        U.bootstrap_significance(np.zeros(16), np.zeros(17), 16000.0, rng="device")
    with pytest.raises(ValueError):
        U.bootstrap_significance(np.zeros(16), np.zeros(16), 16000.0, rng="mersenne")
