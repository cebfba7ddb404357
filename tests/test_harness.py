"""The harness's own comparisons (tests/harness.py), on the CPU: the helpers every bit-for-bit GPU test now
shares fail when they should, and say where."""
import numpy as np
import pytest

from harness import assert_equal, float_bits, same_bytes, words_to_bytes


def test_word_comparison_names_the_one_differing_word():
    ref = np.arange(6 * 5, dtype=np.int32).reshape(6, 5)
    assert_equal(ref.copy(), ref, "equal")
    got = ref.copy()
    got[4, 3] ^= 1 << 24   # one bit of one word
    with pytest.raises(AssertionError) as e:
        assert_equal(got, ref, "frame 7")
    assert e.value.args[0] == ("frame 7", 1, [[4, 3]])


def test_word_comparison_reports_the_first_five_and_the_count():
    ref = np.zeros((3, 4), np.int32)
    got = ref.copy()
    got[1:] = 9
    with pytest.raises(AssertionError) as e:
        assert_equal(got, ref, "band")
    assert e.value.args[0] == ("band", 8, [[1, 0], [1, 1], [1, 2], [1, 3], [2, 0]])


def test_word_comparison_rejects_another_shape():
    with pytest.raises(AssertionError):
        assert_equal(np.zeros((2, 4), np.int32), np.zeros((1, 4), np.int32), "band")   # would broadcast


def test_float_bits_tell_zeros_and_nan_payloads_apart():
    zeros = np.array([0.0, -0.0], np.float32)
    assert zeros[0] == zeros[1] and float_bits(zeros).tolist() == [0, 0x80000000]
    nans = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(np.float32)
    assert np.isnan(nans).all() and float_bits(nans).tolist() == [0x7FC00000, 0x7FC00001]
    with pytest.raises(AssertionError) as e:
        assert_equal(float_bits(nans[:1]), float_bits(nans[1:]), "payload")
    assert e.value.args[0] == ("payload", 1, [[0]])
    assert_equal(float_bits(nans), float_bits(nans.copy()), "the same NaNs are equal as bits")
    assert float_bits(np.float32(-0.0)).tolist() == [0x80000000]                    # a scalar
    strided = np.arange(8, dtype=np.float32)[::2]
    assert float_bits(strided).tolist() == float_bits(strided.copy()).tolist()      # made contiguous


def test_words_to_bytes_round_trips():
    rng = np.random.default_rng(5)
    words = rng.integers(-2 ** 31, 2 ** 31, (7, 3), dtype=np.int64).astype(np.int32)
    b = words_to_bytes(words)
    assert b.shape == (7, 3, 4) and b.dtype == np.uint8
    assert np.array_equal(b.reshape(7, 12).view(np.int32), words)
    assert b[2, 1].tolist() == [(int(words[2, 1]) >> s) & 0xFF for s in (0, 8, 16, 24)]   # R, G, B, A: little-endian
    assert same_bytes(b, words) and not same_bytes(b, words + 1)
    assert np.array_equal(words_to_bytes(words[:, ::2]), b[:, ::2])   # not contiguous: copied first
