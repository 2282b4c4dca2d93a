"""Bit image of a panel's {0, 1} columns (DevicePanel.bits1; data/device_dgp.bits1_index is
the host twin of csrc/dgp.hip x1_byte / x1_bit): the order is a bijection of the 128 x 64
cells of a 64-row block onto the 8,192 bits of its 1 KB image, pack and unpack invert each
other, every MFMA lane's bits of a 64-column plane are 8 contiguous bytes, and the Gram
kernel's widening (csrc/gram.hip bits_rep / bits_to_bf16x8: one shift and one AND per
fragment dword) yields exactly the lane's rows."""
import numpy as np
import pytest

from ate_replication_causalml_amd.data.device_dgp import (BITS_BLOCK, bits1_index,
                                                          pack_bits_block, unpack_bits_block)

COLS, ROWS = np.arange(128)[:, None], np.arange(64)[None, :]


def test_every_cell_maps_to_exactly_one_bit():
    byte, bit = bits1_index(COLS, ROWS)
    assert byte.shape == bit.shape == (128, 64)
    assert byte.min() == 0 and byte.max() == BITS_BLOCK - 1 and bit.min() == 0 and bit.max() == 7
    flat = (byte * 8 + bit).reshape(-1)
    assert np.array_equal(np.sort(flat), np.arange(BITS_BLOCK * 8))


def test_pack_unpack_round_trip():
    rs = np.random.RandomState(5)
    block = rs.randint(0, 2, size=(128, 64)).astype(np.uint8)
    image = pack_bits_block(block)
    assert image.dtype == np.uint8 and image.shape == (BITS_BLOCK,)
    assert np.array_equal(unpack_bits_block(image), block)
    # the other way: any image is the pack of its unpacking
    image2 = rs.randint(0, 256, size=BITS_BLOCK).astype(np.uint8)
    assert np.array_equal(pack_bits_block(unpack_bits_block(image2)), image2)
    # non-zero counts as one (the byte copy marks a one with 0x3F)
    assert np.array_equal(pack_bits_block(block * 0x3F), image)
    # single cells: one bit each, where the index says
    for c, r in [(0, 0), (127, 63), (17, 33), (64, 8), (79, 31)]:
        one = np.zeros((128, 64), dtype=np.uint8)
        one[c, r] = 1
        by, bi = bits1_index(c, r)
        want = np.zeros(BITS_BLOCK, dtype=np.uint8)
        want[int(by)] = 1 << int(bi)
        assert np.array_equal(pack_bits_block(one), want)
    with pytest.raises(ValueError):
        pack_bits_block(np.zeros((64, 128)))


def test_lane_bytes_are_contiguous_and_lane_linear():
    """Lane l = 16 r + c15 reads rows 8r..8r+7 and 32+8r..32+8r+7 of columns c15 + 16 k: the
    four column blocks of a plane are the 8 bytes at plane * 512 + 8 l (one ds_read_b64 per
    plane, stride 8 over the lanes)."""
    for lane in range(64):
        r, c15 = lane >> 4, lane & 15
        rows = np.concatenate([np.arange(8 * r, 8 * r + 8), np.arange(32 + 8 * r, 40 + 8 * r)])
        for plane in range(2):
            cols = plane * 64 + c15 + 16 * np.arange(4)
            byte, _ = bits1_index(cols[:, None], rows[None, :])
            assert set(byte.reshape(-1)) == set(range(plane * 512 + 8 * lane,
                                                      plane * 512 + 8 * lane + 8))
            for k in range(4):           # one halfword per 16-column block
                assert set(byte[k]) == {plane * 512 + 8 * lane + 2 * k,
                                        plane * 512 + 8 * lane + 2 * k + 1}


def test_widening_by_shift_and_mask_gives_the_lanes_rows():
    """The kernel's arithmetic on the host: halfword h = lo | hi << 8 replicated as bytes
    [lo, hi, hi, lo]; dword t of the lane's fragments (half t >> 2, rows 2j and 2j + 1 with
    j = t & 3) is (w << (14 - t)) & 0x40004000, i.e. bf16 2.0 (0x4000) where the row is one."""
    rs = np.random.RandomState(9)
    block = rs.randint(0, 2, size=(128, 64)).astype(np.uint8)
    image = pack_bits_block(block)
    for lane in (0, 5, 21, 47, 63):
        r, c15 = lane >> 4, lane & 15
        for col in (c15, 16 + c15, 64 + c15, 112 + c15):
            off = (col >> 6) * 512 + lane * 8 + ((col >> 4) & 3) * 2
            lo, hi = int(image[off]), int(image[off + 1])
            w = lo | hi << 8 | hi << 16 | lo << 24
            for t in range(8):
                d = ((w << (14 - t)) & 0xFFFFFFFF) & 0x40004000
                half, j = t >> 2, t & 3
                row = 32 * half + 8 * r + 2 * j
                assert d & 0xFFFF == (0x4000 if block[col, row] else 0)
                assert d >> 16 == (0x4000 if block[col, row + 1] else 0)
