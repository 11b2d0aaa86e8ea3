"""The library's one definition of a solid voxel (csrc/dxv_solid.h: the byte is non-zero) on the CPU: the header compiled with g++
(tests/solid_host.py) against numpy and nothing else -- np.packbits(bytes != 0, bitorder="little") for the masks, np.count_nonzero for
the counts -- on every word of the bytes a 0 / 1 shortcut gets wrong, on every value of every byte position, and on ragged ends."""
import numpy as np
import pytest

import solid_host as sh

EDGE = np.array([0x00, 0x01, 0x02, 0x03, 0x7F, 0x80, 0xFE, 0xFF], np.uint8)


def check_words(byte_rows):
    """byte_rows: uint8 [n, 8], byte k of row i = bits 8k .. 8k+7 of word i"""
    byte_rows = np.ascontiguousarray(byte_rows, np.uint8)
    w = byte_rows.view("<u8").reshape(-1)
    bits, marks = sh.words(w)
    want = np.packbits(byte_rows != 0, axis=1, bitorder="little").reshape(-1)
    assert np.array_equal(bits, want)
    assert np.array_equal(marks.astype("<u8").view(np.uint8).reshape(-1, 8), np.where(byte_rows != 0, 0x80, 0).astype(np.uint8))


def test_every_word_of_the_edge_bytes():
    """all 8^8 words whose bytes come from {00, 01, 02, 03, 7F, 80, FE, FF}, a quarter at a time"""
    low = np.stack(np.meshgrid(*[EDGE] * 7, indexing="ij"), axis=-1).reshape(-1, 7)      # 8^7 rows: bytes 1 .. 7
    for first in EDGE:
        rows = np.empty((len(low), 8), np.uint8)
        rows[:, 0] = first
        rows[:, 1:] = low
        check_words(rows)


@pytest.mark.parametrize("background", [0x00, 0xFF])
def test_every_value_of_every_byte_position(background):
    rows = np.full((8, 256, 8), background, np.uint8)
    for k in range(8):
        rows[k, :, k] = np.arange(256)
    check_words(rows.reshape(-1, 8))


def test_seeded_random_words():
    rng = np.random.default_rng(20)
    rows = rng.integers(0, 256, (1 << 16, 8), dtype=np.uint8)
    rows[rng.random(rows.shape) < 0.5] = 0
    check_words(rows)


def tail_cases(n, rng):
    yield np.zeros(n, np.uint8)
    for value in (0x01, 0x02, 0x80, 0xFE, 0xFF):
        yield np.full(n, value, np.uint8)
        one = np.zeros(n, np.uint8)
        one[n - 1] = value                                              # only the last byte: the bit a tail drops first
        yield one
    for _ in range(32):
        g = rng.choice(EDGE, n)
        g[rng.random(n) < 0.4] = 0
        yield g


@pytest.mark.parametrize("n", range(1, 16))
def test_scalar_form_on_every_tail_length(n):
    rng = np.random.default_rng(100 + n)
    for g in tail_cases(n, rng):
        want = np.packbits(g != 0, bitorder="little")
        assert sh.tail_bits(g) == int(want[0]), (n, g)                  # the first eight bytes at the most, zero bits behind the run
        if n > 8:
            assert sh.tail_bits(g[8:]) == int(want[1]), (n, g)
        packed, count = sh.pack_and_count(g)                            # n < 16: the kernels' tail path alone
        assert np.array_equal(packed, want) and count == int(np.count_nonzero(g)), (n, g)


@pytest.mark.parametrize("n", [16, 17, 31, 32, 108, 700, 4096 + 9])
def test_body_and_tail_agree_in_the_kernels_order(n):
    rng = np.random.default_rng(n)
    for g in tail_cases(n, rng):
        packed, count = sh.pack_and_count(g)
        assert np.array_equal(packed, np.packbits(g != 0, bitorder="little")), n
        assert count == int(np.count_nonzero(g)), n
