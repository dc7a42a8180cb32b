"""Writes iq4xs_blocks.json beside itself: known-answer super-blocks for the IQ4_XS twin of tests/iq4xs_ref.py.

A worksheet, not a decoder: every block is laid out value by value with scalar loops from the layout description in DESIGN.md 4g, and the 256 expected
floats are written down from the (scale, table index) that were PUT at each position - nothing is read back from the bytes.  All d are powers of two and
all products are integers below 2^13, so the expected values are exact in float32 whatever the order of operations.  It imports nothing from tests/."""
import json
import os
import struct

TABLE = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]


def f16_bytes(x):
    return list(struct.pack("<e", x))


def iq4xs(scale6, index, d):
    """scale6[8] in 0..63 (used as scale6 - 32), index[256] in 0..15 (into TABLE)"""
    raw = [0] * 136
    raw[0:2] = f16_bytes(d)
    for ib in range(8):  # low four bits: a nibble of scales_l, two sub-blocks a byte, the even one low; upper two bits: a bit pair of the 16-bit scales_h
        raw[4 + ib // 2] |= (scale6[ib] & 15) << (4 * (ib % 2))
        h = (scale6[ib] >> 4) << (2 * ib)
        raw[2] |= h & 0xFF
        raw[3] |= h >> 8
    for i in range(256):  # value 32 ib + j: byte 16 ib + j % 16 of qs, low nibble for j < 16, high nibble for j >= 16
        ib, j = i // 32, i % 32
        raw[8 + 16 * ib + j % 16] |= index[i] << (4 if j >= 16 else 0)
    want = [d * (scale6[i // 32] - 32) * TABLE[index[i]] for i in range(256)]
    return {"type": "iq4_xs", "bytes": raw, "values": want}


blocks = [
    dict(iq4xs([0] * 8, [0] * 256, 0.5), name="every scale and index at its minimum (-32 x -127 in every position)"),
    dict(iq4xs([63] * 8, [15] * 256, 0.5), name="every scale and index at its maximum (31 x 113)"),
    # 5, 58, 23, 40, 14, 49, 31, 0: the low nibbles 5, 10, 7, 8, 14, 1, 15, 0 all differ, and the bit pairs 0, 3, 1, 2, 0, 3, 1, 0 differ between neighbours
    dict(iq4xs([5, 58, 23, 40, 14, 49, 31, 0], [(7 * i + i // 32) % 16 for i in range(256)], 0.125), name="a different scale in every sub-block"),
    # index = j % 16 for the low-nibble values and 15 - j % 16 for the high ones: a swapped nibble half or a byte shifted by one changes every value
    dict(iq4xs([33] * 8, [(i % 16) if (i % 32) < 16 else 15 - (i % 16) for i in range(256)], 1.0), name="an index ramp up the low nibbles and down the high ones"),
    dict(iq4xs([9 * ib for ib in range(8)], [(5 * i + 3) % 16 for i in range(256)], -0.25), name="negative d"),
    dict(iq4xs([63 - 9 * ib for ib in range(8)], [(11 * i) % 16 for i in range(256)], 2.0 ** -24), name="f16-subnormal d (the smallest one)"),
]

if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "iq4xs_blocks.json"), "w") as f:
        json.dump(blocks, f, separators=(",", ":"))
        f.write("\n")
