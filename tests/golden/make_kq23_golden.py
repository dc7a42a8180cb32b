"""Writes kq23_blocks.json beside itself: known-answer super-blocks for the Q2_K / Q3_K twin of tests/kq23_ref.py.

A worksheet, not a decoder: every block is laid out value by value with scalar loops from the layout description in DESIGN.md 4e, and the 256 expected
floats are written down from the (scale, min, level) that were PUT at each position - nothing is read back from the bytes.  All d / dmin are powers of two and
all products are small integers, so the expected values are exact in float32 whatever the order of operations.  It imports nothing from tests/."""
import json
import os
import struct


def f16_bytes(x):
    return list(struct.pack("<e", x))


def sub_block(i):  # value i = 128 n + 32 j + l lives in sub-block 8 n + 2 j + l // 16
    n, j, l = i // 128, (i // 32) % 4, i % 32
    return 8 * n + 2 * j + l // 16


def q2k(scale, mn, level, d, dmin):
    """scale[16], mn[16] in 0..15, level[256] in 0..3"""
    raw = [0] * 84
    for s in range(16):
        raw[s] = scale[s] | (mn[s] << 4)
    for i in range(256):
        n, j, l = i // 128, (i // 32) % 4, i % 32
        raw[16 + 32 * n + l] |= level[i] << (2 * j)
    raw[80:82] = f16_bytes(d)
    raw[82:84] = f16_bytes(dmin)
    want = [d * scale[sub_block(i)] * level[i] - dmin * mn[sub_block(i)] for i in range(256)]
    return {"type": "q2_K", "bytes": raw, "values": want}


def q3k(scale6, level, d):
    """scale6[16] in 0..63 (used as scale6 - 32), level[256] in -4..3"""
    raw = [0] * 110
    for i in range(256):
        n, j, l = i // 128, (i // 32) % 4, i % 32
        low2 = level[i] + 4 if level[i] < 0 else level[i]
        raw[32 + 32 * n + l] |= low2 << (2 * j)
        if level[i] >= 0:  # a SET bit means "nothing subtracted"
            raw[l] |= 1 << (4 * n + j)
    for s in range(16):  # low four bits: bytes 0..7, scales s and s + 8 share a byte; upper two bits: bytes 8..11, four scales a byte
        if s < 8:
            raw[96 + s] |= scale6[s] & 15
        else:
            raw[96 + s - 8] |= (scale6[s] & 15) << 4
        raw[96 + 8 + s % 4] |= (scale6[s] >> 4) << (2 * (s // 4))
    raw[108:110] = f16_bytes(d)
    want = [d * (scale6[sub_block(i)] - 32) * level[i] for i in range(256)]
    return {"type": "q3_K", "bytes": raw, "values": want}


blocks = [
    dict(q2k([0] * 16, [0] * 16, [0] * 256, 0.5, 0.25), name="q2_K every scale, min and level at its minimum"),
    dict(q2k([15] * 16, [15] * 16, [3] * 256, 0.5, 0.25), name="q2_K every scale, min and level at its maximum"),
    dict(q2k(list(range(16)), [15 - s for s in range(16)], [(7 * i + i // 16) % 4 for i in range(256)], 0.125, 0.0625), name="q2_K a different scale in every sub-block"),
    dict(q3k([0] * 16, [-4] * 256, 0.5), name="q3_K every scale and level at its minimum (-32 x -4 in every position)"),
    dict(q3k([63] * 16, [3] * 256, 0.5), name="q3_K every scale and level at its maximum"),
    dict(q3k([4 * s + 1 for s in range(16)], [(5 * i + i // 16) % 8 - 4 for i in range(256)], -0.25), name="q3_K a different scale in every sub-block, negative d"),
]
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kq23_blocks.json")
with open(out, "w") as f:
    json.dump(blocks, f, separators=(",", ":"))
    f.write("\n")
print(out, len(blocks))
