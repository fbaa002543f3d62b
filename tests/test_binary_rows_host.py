"""Bit rows (SCANN_HIP_ROWS_BIN1 / SCANN_HIP_HAMMING), the parts that need no GPU: the packing helpers of hip.py and
the two constants against the header."""
import os
import re

import numpy as np
import pytest

from scann_rust_amd import hip

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "scann_hip.h")


@pytest.mark.parametrize("shape", [(1, 1), (5, 8), (3, 31), (4, 33), (2, 3, 70), (7, 256)])
def test_pack_unpack_round_trip(shape):
    bits = np.random.default_rng(shape[-1]).random(shape) < 0.5
    packed = hip.pack_bits(bits)
    assert packed.dtype == np.uint8 and packed.shape == shape[:-1] + ((shape[-1] + 7) // 8,)
    assert np.array_equal(hip.unpack_bits(packed, shape[-1]), bits.astype(np.uint8))
    for j in range(8 * packed.shape[-1]):   # element j is bit j & 7 of byte j >> 3, pad bits clear
        assert np.array_equal((packed[..., j >> 3] >> (j & 7)) & 1, bits[..., j] if j < shape[-1] else np.zeros(shape[:-1]))
    assert np.array_equal(hip.pack_bits(bits.astype(np.float32) * 2.5), packed)   # anything != 0 is a one


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.search(r"#define SCANN_HIP_ROWS_BIN1 (\d+)", text).group(1)) == hip.ROWS_BIN1 == 6
    assert int(re.search(r"SCANN_HIP_HAMMING = (\d+)", text).group(1)) == hip.HAMMING == 5
    assert not re.search(r"#define SCANN_HIP_ROWS_\w+ 4\b", text)   # value 4 stays unused
