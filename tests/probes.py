"""Read-out weights and edge activations: builders shared by test_readout_probes.py (CPU) and test_gpu_value_edges.py (GPU).

A weight matrix whose row j de-quantises to the unit vector e_j turns a quantised mat-mul into a read-out of its own activation
quantiser: output (m, j) = d_act * q_act[j] — one non-zero term, every other term an exact zero, so the f32 result does not depend
on summation order, tiling, K split or MFMA shape.  A second matrix (Q4_K / Q5_K only) reads the Q8_K `bsums` field the same way
through the mins term: all nibbles 0, dmin = 1, one six-bit min = 1 -> output = -d_act * (bsums[2s] + bsums[2s + 1]).

The expected values come from the NumPy restatement of the two activation quantisers in tests/golden/make_golden.py — the second
reference beside the C oracle.
"""
import os
import sys

import numpy as np

import llama_box_amd as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as MG  # noqa: E402

F16_ONE = np.array([1.0], np.float16).view(np.uint8)
KQ = (L.Q4_K, L.Q5_K, L.Q6_K)


def act_kind(qt):
    return "q8_0" if qt == L.Q8_0 else "q8_K"


def pack_scales_k4(sc, mn):
    """Eight six-bit scales and mins -> the 12 packed bytes of a Q4_K / Q5_K block (inverse of make_golden.scale_min_k4)."""
    sc = np.asarray(sc, np.uint8)
    mn = np.asarray(mn, np.uint8)
    out = np.zeros(12, np.uint8)
    for j in range(4):
        out[j] = (sc[j] & 63) | ((sc[j + 4] >> 4) << 6)
        out[4 + j] = (mn[j] & 63) | ((mn[j + 4] >> 4) << 6)
        out[8 + j] = (sc[j + 4] & 0xF) | ((mn[j + 4] & 0xF) << 4)
    return out


def zero_block(qt):
    """The block of `qt` whose 256 (32) values are all zero with a live scale: d = 1, scales 1, quants at their zero point."""
    b = np.zeros(L.TYPE_SIZE[qt], np.uint8)
    if qt == L.Q8_0:
        b[0:2] = F16_ONE
    elif qt in (L.Q4_K, L.Q5_K):
        b[0:2] = F16_ONE
        b[4:16] = pack_scales_k4([1] * 8, [0] * 8)
    elif qt == L.Q6_K:
        b[128:192] = 0xAA  # the two high bits of every quant = 2 -> 32 -> value 0
        b[192:208] = 1
        b[208:210] = F16_ONE
    else:
        raise ValueError(qt)
    return b


def one_hot_block(qt, e):
    """zero_block(qt) with the value 1 at element e."""
    b = zero_block(qt)
    if qt == L.Q8_0:
        b[2 + e] = 1
    elif qt in (L.Q4_K, L.Q5_K):
        qs = 48 if qt == L.Q5_K else 16
        j, r = divmod(e, 64)
        b[qs + 32 * j + (r % 32)] = 1 if r < 32 else 0x10
    else:
        h, r = divmod(e, 128)
        g, l = divmod(r, 32)
        b[64 * h + 32 * (g & 1) + l] = 1 if g < 2 else 0x10
    return b


def readout_weight(qt, K):
    """Raw bytes of the [K, K] matrix whose row j de-quantises to e_j."""
    blck, bs = L.TYPE_BLCK[qt], L.TYPE_SIZE[qt]
    assert K % blck == 0
    nb = K // blck
    w = np.tile(zero_block(qt), (K, nb)).reshape(K, nb, bs)
    hot = np.stack([one_hot_block(qt, e) for e in range(blck)])
    for j in range(K):
        w[j, j // blck] = hot[j % blck]
    return np.ascontiguousarray(w.reshape(K, nb * bs))


def bsums_readout_weight(qt, K):
    """Raw bytes of the [K, K/32] matrix (Q4_K / Q5_K) whose row r = 8 * block + s has dmin = 1 and the one min s = 1 in that block, every nibble 0."""
    assert qt in (L.Q4_K, L.Q5_K) and K % 256 == 0
    bs = L.TYPE_SIZE[qt]
    nb = K // 256
    w = np.tile(zero_block(qt), (K // 32, nb)).reshape(K // 32, nb, bs)
    for r in range(K // 32):
        blk, s = divmod(r, 8)
        b = np.zeros(bs, np.uint8)
        b[0:2] = F16_ONE
        b[2:4] = F16_ONE
        mn = [0] * 8
        mn[s] = 1
        b[4:16] = pack_scales_k4([1] * 8, mn)
        w[r, blk] = b
    return np.ascontiguousarray(w.reshape(K // 32, nb * bs))


# ------------------------------------------------------------------------------------------------ edge activations
def _filler(rng, n, lim=4.0):
    return np.clip(rng.standard_normal(n) * 1.5, -lim, lim).astype(np.float32)


def edge_blocks(kind, rng):
    """[(name, block)] — one planted block (256 values for q8_K, 32 for q8_0) per property."""
    B = 256 if kind == "q8_K" else 32
    f32 = np.float32
    out = []

    def add(name, v):
        v = np.asarray(v, np.float32)
        assert v.shape == (B,), (name, v.shape)
        out.append((name, v))

    # 1. half-way everywhere: integers + 0.5 with one element +-127, so the scale is exactly -+1 (Q8_K) / 1 (Q8_0)
    for name, top in (("halfway_max_pos", 127.0), ("halfway_max_neg", -127.0)):
        v = rng.integers(-127, 127, B).astype(np.float32) + f32(0.5)
        v[int(rng.integers(0, B))] = top
        add(name, v)
    # 2. tie for max|x|: negative first / positive later and the mirror; in different groups of four and inside one
    far = (10, 200) if B == 256 else (2, 29)
    for name, (i, j), first in (("tie_neg_first_far", far, -5.0), ("tie_pos_first_far", far, 5.0), ("tie_neg_first_quad", (8, 10), -5.0), ("tie_pos_first_quad", (8, 10), 5.0)):
        v = _filler(rng, B)
        v[i], v[j] = first, -first
        add(name, v)
    # 3. the maximum on the last element / on the first
    v = _filler(rng, B)
    v[B - 1] = 7.3
    add("max_last", v)
    v = _filler(rng, B)
    v[0] = -7.3
    add("max_first", v)
    # 4. constant blocks: every quant -127 (Q8_K; every bsums entry -2032) and the mirror
    add("const_neg", np.full(B, -3.7, np.float32))
    add("const_pos", np.full(B, 3.7, np.float32))
    # 5. the clamp and its neighbours
    c = f32(3.7)
    v = _filler(rng, B, 3.0)
    v[3], v[20], v[21], v[22] = -c, c, np.nextafter(c, f32(0)), np.nextafter(-c, f32(0))
    add("clamp_inner", v)
    v = _filler(rng, B, 3.0)
    v[3], v[20], v[21], v[22] = -c, np.nextafter(c, f32(np.inf)), c, np.nextafter(-c, f32(-np.inf))
    add("clamp_outer", v)
    v = np.full(B, 3.7, np.float32)
    v[0] = -c
    add("clamp_all_but_first", v)  # Q8_K: q[0] = -127, every other quant +127
    # 6. both zeros mixed; zeros among values
    v = np.zeros(B, np.float32)
    v[1::2] = -0.0
    add("zeros_mixed", v)
    v = _filler(rng, B)
    v[0::3] = 0.0
    v[1::6] = -0.0
    add("zeros_among_values", v)
    # 7. f32 subnormals (Q8_K: iscale overflows to inf in the reference), subnormal values under a normal maximum, and 1e30 (Q8_K only: a Q8_0 scale above
    #    the f16 range is inf, and the read-out's zero terms would turn into NaN)
    add("subnormal", rng.integers(-100, 101, B).astype(np.float32) * f32(1e-41))
    v = rng.integers(-11, 12, B).astype(np.float32) * f32(1e-39)
    v[int(rng.integers(0, B))] = f32(4e-37)
    add("subnormal_under_normal_max", v)
    if kind == "q8_K":
        add("huge_1e30", _filler(rng, B) * f32(1e30))
    return out


def edge_activations(kind, K, rng):
    """-> (rows float32 [n, K], names).  Row i carries planted block i of edge_blocks at block index (3 * i + 1) % (K / B) — a different
    block per row — over Gaussian filler; 'zero_block_neighbour' rows and plain Gaussian rows (the old regime) follow."""
    B = 256 if kind == "q8_K" else 32
    assert K % B == 0
    nb = K // B
    blocks = edge_blocks(kind, rng)
    rows, names = [], []
    for i, (name, v) in enumerate(blocks):
        r = (rng.standard_normal(K) * rng.uniform(0.2, 3.0)).astype(np.float32)
        at = (3 * i + 1) % nb
        r[at * B:(at + 1) * B] = v
        rows.append(r)
        names.append(f"{name}@{at}")
    r = (rng.standard_normal(K) * 2.0).astype(np.float32)
    at = nb // 2
    r[at * B:(at + 1) * B] = 0.0
    rows.append(r)
    names.append(f"zero_block_neighbour@{at}")
    for g in range(3):
        rows.append((rng.standard_normal(K) * rng.uniform(0.2, 3.0)).astype(np.float32))
        names.append(f"gaussian{g}")
    return np.stack(rows), names


def tile_rows(x, M):
    """M rows cycling through the catalogue x (every row of x appears when M >= len(x))."""
    return np.ascontiguousarray(x[np.arange(M) % x.shape[0]])


# ------------------------------------------------------------------------------------------------ expected values (NumPy twins)
def quantize(kind, x, q8K=MG.quantize_q8_K, q80=MG.quantize_q8_0):
    """x [n, K] -> (d float32 [n, K/B], q int32 [n, K/B, B], bsums int32 [n, K/256, 16] or None) by the NumPy twin (or a mutant of it)."""
    n, K = x.shape
    with np.errstate(all="ignore"):
        if kind == "q8_K":
            d, q, bs = q8K(x.reshape(-1, 256))
            return d.astype(np.float32).reshape(n, -1), q.astype(np.int32).reshape(n, -1, 256), bs.astype(np.int32).reshape(n, -1, 16)
        d, q = q80(x.reshape(-1, 32))
        return d.astype(np.float32).reshape(n, -1), q.astype(np.int32).reshape(n, -1, 32), None


def expected_readout(kind, x, **twins):
    """What MUL_MAT(readout_weight, x) must return: d_act * q_act, one f32 product per element."""
    d, q, _ = quantize(kind, x, **twins)
    with np.errstate(all="ignore"):
        return (d[:, :, None] * q.astype(np.float32)).astype(np.float32).reshape(x.shape)


def expected_bsums_readout(x, **twins):
    """What MUL_MAT(bsums_readout_weight, x) must return: -d_act * (bsums[2s] + bsums[2s + 1]) per 32-value sub-block."""
    d, _, bs = quantize("q8_K", x, **twins)
    pair = bs.reshape(bs.shape[0], bs.shape[1], 8, 2).sum(axis=3).astype(np.float32)
    with np.errstate(all="ignore"):
        return (-(d[:, :, None] * pair)).astype(np.float32).reshape(x.shape[0], -1)


def bits(a):
    """f32 -> uint32 with -0.0 folded onto +0.0 and every NaN onto one pattern: the equality the read-out gates use."""
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    u = a.view(np.uint32).copy()
    u[a == 0] = 0
    u[np.isnan(a)] = 0x7FC00000
    return u
