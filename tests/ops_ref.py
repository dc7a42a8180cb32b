"""NumPy twins of the generic ops of csrc/ops.hip, written from the op DEFINITIONS (ggml.h's statement of each op and the published
formulas), not from oracle/ggml_cpu_ref.c — a second reference beside the C oracle, so that a misreading shared by kernel and oracle
does not pass.  tests/test_ops_ref_host.py pins twin and oracle to each other on the CPU; tests/test_gpu_ops_edges.py judges the kernels.

Arrays are in NumPy order (the reverse of ggml's ne[]): a ggml tensor [ne0, ne1, ne2, ne3] is an array of shape (ne3, ne2, ne1, ne0).

Two flavours:
  * f32 step for step — ops whose contract is bit equality (binary, scale, RELU, NEG, clamp, cpy / cast, get_rows, set_rows, argmax): every
    operation is one IEEE f32 operation in NumPy, in the order the definition states.
  * float64 — ops compared by distance (rms_norm, silu / exp / tanh / sigmoid, swiglu, soft_max, rope).  Where the DEFINITION fixes an f32
    intermediate whose range or value the result depends on (the f32 squares of rms_norm, expf's f32 overflow inside silu / sigmoid, rope's
    chain of f32 multiplies for the angle, soft_max's f32 logits) the twin computes that intermediate in f32 and everything after it in float64.
"""
import functools
import os
import re

import numpy as np

import llama_box_amd as L

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
UNARY = {"NEG": 2, "TANH": 4, "RELU": 6, "SIGMOID": 7, "SILU": 10, "EXP": 13}  # enum ggml_unary_op (include/ggml_abi.h)
UNARY_BITS = ("RELU", "NEG")
EXPF_HI, EXPF_LO = 88.72283905206835, -103.97207708399179  # expf's range ends: above -> inf, below -> 0 (ln FLT_MAX, ln 2^-150)


# ------------------------------------------------------------------------------------------------ distances
def f32_ulp(ref64):
    """The f32 unit in the last place at |ref| (2^-149 below FLT_MIN; the top binade's for anything larger)."""
    a = np.minimum(np.abs(np.asarray(ref64, np.float64)), float(FLT_MAX))
    a = np.where(np.isfinite(a), a, float(FLT_MAX))
    _, e = np.frexp(a)
    e = np.where(a == 0, -125, e)  # (frexp(0) has exponent 0: the unit at zero is the subnormal step)
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def ulp_distance(got_f32, ref_f64):
    """|got - ref| in f32 ulps at ref, element by element.  Equal values (both NaN, the same infinity — also where ref overflows f32 —
    or the same number) are 0; a NaN or an infinity on one side only is inf, and so is a zero of the other sign than an exactly zero ref."""
    got = np.asarray(got_f32, np.float32).astype(np.float64)
    ref = np.asarray(ref_f64, np.float64)
    with np.errstate(all="ignore"):
        r32 = ref.astype(np.float32).astype(np.float64)
        d = np.abs(got - ref) / f32_ulp(ref)
    same = (np.isnan(got) & np.isnan(ref)) | (got == r32) | (got == ref)
    d = np.where(same, 0.0, d)
    d = np.where((got == 0) & (ref == 0) & (np.signbit(got) != np.signbit(ref)), np.inf, d)
    return np.where(np.isnan(d), np.inf, d)


def row_distance(got, ref_f64, scale=None):
    """max |got - ref| per row over that row's largest |ref| (or over `scale`, one value per row): the measure for soft_max and rope, where
    cancellation makes ulps meaningless near zero.  Rows that are NaN on both sides count 0."""
    got = np.asarray(got).astype(np.float64)
    ref = np.asarray(ref_f64, np.float64)
    both_nan = np.isnan(got) & np.isnan(ref)
    g, r = np.where(both_nan, 0.0, got), np.where(both_nan, 0.0, ref)
    with np.errstate(all="ignore"):
        den = np.max(np.abs(r), axis=-1) if scale is None else np.asarray(scale, np.float64)
        den = np.where(den > 0, den, 1.0)
        d = np.max(np.abs(g - r), axis=-1) / den
    return np.where(np.isnan(d), np.inf, d)


def bits(a):
    """f32 -> uint32 / f16 -> uint16 / integers as they are, every NaN folded onto one pattern (NaNs are compared by isnan, the rest by bits)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = 0x7FC00000
        return u
    if a.dtype == np.float16:
        u = a.view(np.uint16).copy()
        u[np.isnan(a)] = 0x7E00
        return u
    return a


# ------------------------------------------------------------------------------------------------ value catalogue
def catalogue():
    """The f32 values at which conversions, comparisons and expf change behaviour (in the manner of probes.py's edge blocks)."""
    up, dn = f32(np.inf), f32(-np.inf)
    v = [0.0, -0.0, 1.0, -1.0, 0.5, 3.0]
    sub_min, sub_max = f32(2.0 ** -149), np.nextafter(FLT_MIN, f32(0))
    v += [sub_min, -sub_min, sub_max, -sub_max, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan]
    # the f16 overflow boundary: 65504 is the largest f16, 65520 the first value that rounds to inf (a tie that goes to the even "2048 * 32")
    v += [65504.0, np.nextafter(f32(65520.0), dn), 65520.0, np.nextafter(f32(65520.0), up), -65504.0, -65520.0, np.nextafter(f32(-65520.0), up)]
    # half a subnormal-f16 step (2^-25: a tie that goes to zero) and its neighbours; the ties at 1.5 and 2.5 steps (-> 2 steps both)
    h = f32(2.0 ** -25)
    v += [h, np.nextafter(h, up), np.nextafter(h, dn), -h, -np.nextafter(h, up), f32(1.5 * 2.0 ** -24), f32(2.5 * 2.0 ** -24), f32(2.0 ** -24), f32(2.0 ** -14), np.nextafter(f32(2.0 ** -14), dn)]
    # f16 ties in the normal range: 1 + 2^-11 (-> 1, even), 1 + 3 * 2^-11 (-> 1 + 2^-9)
    v += [f32(1.0 + 2.0 ** -11), f32(1.0 + 3 * 2.0 ** -11), np.nextafter(f32(1.0 + 2.0 ** -11), up)]
    # expf's range ends and their neighbours (88.72 / -103.97), the start of its subnormal results (-87.34)
    v += [88.72, 88.73, -88.72, -88.73, -87.33, -87.34, -103.97, -103.98, -103.0, 100.0, -100.0, 1e20, -1e20, 1e-20]
    with np.errstate(all="ignore"):
        return np.array(v, np.float64).astype(np.float32)


def seeded(rng, n, span=100.0):
    """n values spanning +-span: a third uniform, a third normal, a third log-uniform in magnitude."""
    k = n // 3
    a = rng.uniform(-span, span, k)
    b = rng.standard_normal(k) * 3.0
    c = np.exp(rng.uniform(np.log(1e-6), np.log(span), n - 2 * k)) * rng.choice([-1.0, 1.0], n - 2 * k)
    return rng.permutation(np.concatenate([a, b, c])).astype(np.float32)


# ------------------------------------------------------------------------------------------------ twins: bit-exact ops
def tile_to(b, shape):
    """ggml's broadcast: element i of the result reads b[i % b.ne] along every dimension."""
    b = np.asarray(b)
    b = b.reshape((1,) * (len(shape) - b.ndim) + b.shape)
    assert all(s % t == 0 for s, t in zip(shape, b.shape)), (shape, b.shape)
    return np.tile(b, [s // t for s, t in zip(shape, b.shape)])


def binary(op, a, b):
    a = np.asarray(a, np.float32)
    b = tile_to(np.asarray(b, np.float32), a.shape)
    with np.errstate(all="ignore"):
        return {"add": a + b, "sub": a - b, "mul": a * b, "div": a / b}[op].astype(np.float32)


def scale(x, s, bias=0.0):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        p = x * f32(s)
        return (p + f32(bias)).astype(np.float32)


def clamp(x, lo, hi):
    """MAX(MIN(x, hi), lo) with C's `a < b ? a : b`: a NaN becomes hi."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        m = np.where(x < f32(hi), x, f32(hi))
        return np.where(m > f32(lo), m, f32(lo)).astype(np.float32)


def unary(op, x):
    """RELU / NEG in f32 (bit-exact); the others in float64, with expf's f32 range kept where it decides the result."""
    x32 = np.asarray(x, np.float32)
    if op == "RELU":
        return np.where(x32 > 0, x32, f32(0.0)).astype(np.float32)  # (-0.0, NaN -> +0.0)
    if op == "NEG":
        return np.negative(x32)
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        if op == "EXP":
            return np.exp(x)
        if op == "TANH":
            return np.tanh(x)
        e = expf_ranged(-x)
        if op == "SIGMOID":
            return 1.0 / (1.0 + e)
        if op == "SILU":
            return x / (1.0 + e)
    raise ValueError(op)


def expf_ranged(x64):
    """exp in float64 with expf's f32 range: inf above ln FLT_MAX, 0 below ln 2^-150 — inside silu / sigmoid the overflow decides the result
    (silu(-100) = -100 / (1 + inf) = -0, not -3.7e-42)."""
    with np.errstate(all="ignore"):
        e = np.exp(x64)
        e = np.where(e > float(FLT_MAX), np.inf, e)
        return np.where(e < 2.0 ** -150, 0.0, e)


def swiglu(a, b):
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return a / (1.0 + expf_ranged(-a)) * b


def swiglu_halves(x, swapped):
    nc = x.shape[-1] // 2
    lo, hi = x[..., :nc], x[..., nc:]
    return swiglu(hi, lo) if swapped else swiglu(lo, hi)


def cast(x, np_dtype):
    """f32 <-> f16 (IEEE round to nearest even, overflow to inf at 65520, subnormals kept) or a same-type copy."""
    with np.errstate(all="ignore"):
        return np.asarray(x).astype(np_dtype)


def permute(x, ax):
    """ggml_permute(x, ax0..ax3) of a 4-D array in NumPy order: dimension i of the source becomes dimension ax[i] of the result."""
    x = np.asarray(x)
    assert x.ndim == 4
    perm = [0, 0, 0, 0]
    for i in range(4):
        perm[3 - ax[i]] = 3 - i
    return np.transpose(x, perm)


def cpy(x, np_dtype, dst_shape=None):
    """CPY / CONT: the source's elements in logical order, converted, in the destination's shape."""
    out = np.ascontiguousarray(cast(np.ascontiguousarray(x), np_dtype))
    return out.reshape(dst_shape) if dst_shape is not None else out


def get_rows(a, idx):
    """a (ne3 = i12, ne2 = i11, rows, ne0) f32 / f16, idx (i12, i11, i10) int32 -> (i12, i11, i10, ne0) f32: row idx[i12, i11, i10] of matrix (i12, i11)."""
    a = np.asarray(a)
    idx = np.asarray(idx)
    a = a.reshape((1,) * (4 - a.ndim) + a.shape)
    idx = idx.reshape((1,) * (3 - idx.ndim) + idx.shape)
    out = np.empty(idx.shape + (a.shape[-1],), np.float32)
    for i12 in range(idx.shape[0]):
        for i11 in range(idx.shape[1]):
            out[i12, i11] = a[i12, i11][idx[i12, i11]].astype(np.float32)
    return out


def set_rows(dst, src, idx):
    """dst (ne3, ne2, rows, nc) f32 / f16, src (ne3, ne2, n, nc) f32, idx (n2, n1, n) int64, broadcast over ne3 / ne2 -> dst with row idx[...] = convert(src row)."""
    out = np.array(dst, copy=True)
    out = out.reshape((1,) * (4 - out.ndim) + out.shape)
    src = np.asarray(src, np.float32)
    src = src.reshape((1,) * (4 - src.ndim) + src.shape)
    idx = np.asarray(idx)
    idx = idx.reshape((1,) * (3 - idx.ndim) + idx.shape)
    for i3 in range(src.shape[0]):
        for i2 in range(src.shape[1]):
            rows = idx[i3 % idx.shape[0], i2 % idx.shape[1]]
            out[i3, i2][rows] = cast(src[i3, i2], out.dtype)
    return out.reshape(np.shape(dst))


def argmax(x):
    """The FIRST index of the row maximum under a strict `>` scan from -inf: NaNs never win, an all -inf (or all-NaN) row gives 0."""
    x = np.asarray(x, np.float32)
    x = x.reshape(-1, x.shape[-1])
    out = np.zeros(x.shape[0], np.int32)
    for r, row in enumerate(x):
        ok = ~np.isnan(row) & (row > -np.inf)
        if ok.any():
            out[r] = int(np.flatnonzero(ok & (row == row[ok].max()))[0])
    return out


# ------------------------------------------------------------------------------------------------ twins: distance ops
def rms_norm(x, eps, w=None):
    """y = x / sqrt(mean(x^2) + eps) [* w].  The squares are f32 products by definition (a row of 1e20 has an infinite mean and a zero result,
    a row of subnormals a zero mean), their sum and everything after it is float64 here."""
    x32 = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        sq = (x32 * x32).astype(np.float32).astype(np.float64)
        mean = sq.sum(axis=-1, keepdims=True) / x32.shape[-1]
        y = x32.astype(np.float64) * (1.0 / np.sqrt(mean + float(f32(eps))))
        if w is not None:
            y = y * np.asarray(w, np.float32).astype(np.float64)
    return y


def alibi_slopes(n_head, max_bias):
    """slope of head h: m0^(h + 1) below the largest power of two in n_head, m1^(2 (h - that) + 1) from there on; m0 / m1 are f32 values (host powf)."""
    n2 = 1 << int(np.floor(np.log2(n_head)))
    m0 = float(f32(2.0 ** (-max_bias / n2)))
    m1 = float(f32(2.0 ** (-(max_bias / 2.0) / n2)))
    return np.array([m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1) for h in range(n_head)], np.float64)


def soft_max(x, mask=None, scale_=1.0, max_bias=0.0, sinks=None):
    """x (ne3, heads, rows, n); mask (m3, m2, >= rows, n) f16 / f32, broadcast over ne3 / heads; sinks (heads,).
    w = x * scale + slope * mask (f32 steps — exactly, when slope is 1; with ALiBi the slope is a power and w is float64), then
    p = exp(w - max) / sum in float64; a sum that is 0 or NaN becomes -inf (llama-box's zero-sum guard: no abort; a fully masked row is NaN, since -inf - -inf is)."""
    x = np.asarray(x, np.float32)
    x = x.reshape((1,) * (4 - x.ndim) + x.shape)
    n3, nh, nr, n = x.shape
    with np.errstate(all="ignore"):
        w = (x * f32(scale_)).astype(np.float32)
        if mask is not None:
            m = np.asarray(mask)
            m = m.reshape((1,) * (4 - m.ndim) + m.shape)[:, :, :nr, :].astype(np.float32)
            m = np.tile(m, [n3 // m.shape[0], nh // m.shape[1], 1, 1])
            if max_bias > 0.0:
                w = w.astype(np.float64) + alibi_slopes(nh, max_bias)[None, :, None, None] * m.astype(np.float64)
            else:
                w = (w + m).astype(np.float32)
        mx = np.max(w, axis=-1, keepdims=True).astype(np.float64)
        if sinks is not None:
            sk = np.asarray(sinks, np.float32).astype(np.float64)[None, :, None, None]
            mx = np.maximum(mx, sk)
        e = np.exp((w.astype(w.dtype) - mx.astype(w.dtype)).astype(np.float64))
        s = e.sum(axis=-1, keepdims=True)
        if sinks is not None:
            s = s + np.exp(sk - mx)
        s = np.where(np.isnan(s) | (s == 0.0), -np.inf, s)
        return e * (1.0 / s)


def rope_theta_scale(freq_base, n_dims):
    return f32(np.power(np.float64(f32(freq_base)), np.float64(f32(-2.0) / f32(n_dims))))


def rope(x, pos, n_dims, neox, freq_base, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0, n_ctx_orig=8192, ff=None, out_dtype=np.float32):
    """x (ne3, tokens, heads, HD) f32 / f16, pos (tokens,) int32.  Pair ip of a token at position p is rotated by
    theta_ip = p * theta_scale^ip — BY DEFINITION the chain of f32 multiplies `theta *= theta_scale`, which is what a position of 10^6 turns on —
    divided by the frequency factor, mixed by YaRN (f32 steps), then cos / sin and the rotation in float64.  normal: pairs (2 ip, 2 ip + 1);
    NeoX: (ip, ip + n_dims / 2); elements from n_dims on pass through.  Returns float64 (for f16 data: the value BEFORE the final f16 rounding)."""
    x = np.asarray(x)
    x = x.reshape((1,) * (4 - x.ndim) + x.shape)
    x64 = x.astype(np.float64)
    n_pairs = n_dims // 2
    ts = rope_theta_scale(freq_base, n_dims)
    with np.errstate(all="ignore"):
        # ggml_rope_yarn_corr_dims
        def corr_dim(n_rot):
            return n_dims * np.log(n_ctx_orig / (n_rot * 2.0 * np.pi)) / (2.0 * np.log(freq_base))
        c0 = f32(max(0.0, np.floor(corr_dim(beta_fast))))
        c1 = f32(min(n_dims - 1.0, np.ceil(corr_dim(beta_slow))))
        theta = np.empty((len(pos), n_pairs), np.float32)
        t = np.asarray(pos, np.int32).astype(np.float32)
        for ip in range(n_pairs):
            theta[:, ip] = t
            t = (t * ts).astype(np.float32)
        if ff is not None:
            theta = (theta / np.asarray(ff, np.float32)[None, :n_pairs]).astype(np.float32)
        interp = (f32(freq_scale) * theta).astype(np.float32)
        th, mscale = interp, float(f32(attn_factor))
        if ext_factor != 0.0:
            y = ((np.arange(n_pairs, dtype=np.float32) - c0) / np.maximum(f32(0.001), c1 - c0)).astype(np.float32)
            ramp = ((f32(1.0) - np.minimum(f32(1.0), np.maximum(f32(0.0), y))) * f32(ext_factor)).astype(np.float32)[None, :]
            th = ((interp * (f32(1.0) - ramp)).astype(np.float32) + (theta * ramp).astype(np.float32)).astype(np.float32)
            mscale = mscale * (1.0 + float(f32(0.1)) * np.log(1.0 / float(f32(freq_scale))))
        cs = (np.cos(th.astype(np.float64)) * mscale)[None, :, None, :]
        sn = (np.sin(th.astype(np.float64)) * mscale)[None, :, None, :]
        ia = np.arange(n_pairs) if neox else 2 * np.arange(n_pairs)
        ib = ia + n_pairs if neox else ia + 1
        out = x64.copy()
        x0, x1 = x64[..., ia], x64[..., ib]
        out[..., ia] = x0 * cs - x1 * sn
        out[..., ib] = x0 * sn + x1 * cs
    return out


# ------------------------------------------------------------------------------------------------ the constants the shapes come from
def ops_limits():
    """The launcher constants the edge shapes of tests/test_gpu_ops_edges.py are derived from, parsed from csrc/ops.hip (as moe_ref.mmid_limits
    parses launch_mmid): a retuned launcher then names the stale shape instead of silently missing the edge.  If an expression is rewritten, the
    pattern below that names it is the line to edit.
      softmax_reg   values a row may have for k_soft_max_reg<NR>, ascending       `a.ne[0] <= 256 * 4) SM_REG(4)` ..., `a.ne[0] <= 256 * 32`
      grid_cap      {launcher: most workgroups of 256 threads before the grid-stride loop takes a second stride}   `(n + 255) / 256, 2048)`
      vec_trip      f32 values one trip of the float4 loops of k_rms_norm / k_set_rows covers   `i0 += 1024` (float4s)
      glu_chunk     values of one grid.y chunk of k_swiglu                          `(nc + 1023) / 1024`"""
    with open(os.path.join(L.REPO, "llama_box_amd", "csrc", "ops.hip")) as f:
        src = f.read()

    def body(name):
        m = re.search(r"\n(?:void|bool) " + name + r"\(.*?\n}\n", src, re.S)
        assert m, f"{name} not found in ops.hip — edit tests/ops_ref.py: ops_limits"
        return m.group(0)

    def kernel(name):
        m = re.search(r"__global__ void [^\n]*\b" + name + r"\(.*?\n}\n", src, re.S)
        assert m, f"{name} not found in ops.hip — edit tests/ops_ref.py: ops_limits"
        return m.group(0)

    def one(text, pattern, what):
        m = re.findall(pattern, text)
        assert len(set(m)) == 1, f"{what}: pattern {pattern!r} matches {m} — the expression moved, edit tests/ops_ref.py: ops_limits"
        return m[0]

    sm = body("launch_soft_max")
    regs = [(int(a) * int(b), int(nr)) for a, b, nr in re.findall(r"a\.ne\[0\] <= (\d+) \* (\d+)\) SM_REG\((\d+)\)", sm)]
    outer = one(sm, r"a\.ne\[0\] <= (\d+) \* (\d+)\) \{", "soft_max: the register kernels' upper end")
    last = int(one(sm, r"else SM_REG\((\d+)\)", "soft_max: the last register kernel"))
    regs.append((int(outer[0]) * int(outer[1]), last))
    assert len(regs) == 3 and all(n == 256 * nr for n, nr in regs), f"launch_soft_max hand-overs {regs}: a row must fit 256 threads x NR registers"
    caps = {name: int(one(body("launch_" + name), r"\(n \+ 255\) / 256, (\d+)\)", f"grid cap of launch_{name}")) for name in ("scale", "unary", "clamp", "cpy")}
    trips = {k: int(one(kernel(k), r"i0 < n4; i0 \+= (\d+)\)", f"float4 trip of {k}")) * 4 for k in ("k_rms_norm", "k_set_rows")}
    assert trips["k_rms_norm"] == trips["k_set_rows"]
    up, chunk = one(body("launch_swiglu"), r"\(nc \+ (\d+)\) / (\d+)\)", "k_swiglu chunk")
    assert int(up) + 1 == int(chunk)
    per_thread = int(one(kernel("k_swiglu"), r"blockIdx\.y \* 256 \+ threadIdx\.x\) \* (\d+);", "k_swiglu values per thread"))
    assert 256 * per_thread == int(chunk), "k_swiglu: a chunk is 256 threads x the values of one thread"
    return {"softmax_reg": [n for n, _ in regs], "grid_cap": caps, "vec_trip": trips["k_rms_norm"], "glu_chunk": int(chunk)}


# the shapes the issue fixes; test_ops_ref_host.py checks them against ops_limits()
SOFTMAX_N = (1, 1024, 1025, 3072, 3073, 8192, 8193)
STRIDE_N = 2048 * 256 + 257   # scale, unary, clamp: a second, partial stride of the grid-stride loop
CPY_STRIDE_N = 1024 * 1024 + 257
RMS_NE0 = (1, 3, 100, 4096, 4100, 8192)
GLU_NC = (6, 1024, 1028, 2050)
SET_ROWS_NC = (3, 256, 4100)


def shapes_from(lim):
    """What the fixed shapes above must be for the constants `lim` (ops_limits())."""
    h = lim["softmax_reg"]
    return {
        "SOFTMAX_N": (1,) + tuple(v for n in h for v in (n, n + 1)),
        "STRIDE_N": {k: lim["grid_cap"][k] * 256 + 257 for k in ("scale", "unary", "clamp")},
        "CPY_STRIDE_N": lim["grid_cap"]["cpy"] * 256 + 257,
        "RMS_NE0": (1, 3, 100, lim["vec_trip"], lim["vec_trip"] + 4, 2 * lim["vec_trip"]),
        "GLU_NC": (6, lim["glu_chunk"], lim["glu_chunk"] + 4, 2 * lim["glu_chunk"] + 2),
        "SET_ROWS_NC": (3, 256, lim["vec_trip"] + 4),
    }


# ------------------------------------------------------------------------------------------------ gates of the distance ops
U24 = 2.0 ** -24  # a relative perturbation r of a result is at most r / 2^-24 of its ulps
# What a kernel may be further from the float64 twin than the ORACLE is on the same inputs (the baseline, measured on the CPU).  Units: f32 ulps of the result
# for "ulp" families, a fraction of the row's largest magnitude for "row" families.  Only what DIFFERS between kernel and oracle is counted; the roundings
# both perform (sqrtf, reciprocals, products, sums) are in the baseline already.
#   rms_norm  only + - x / sqrtf: the one difference is the ORDER of the double partial sums, which can move the f32 mean onto its neighbour, <= 2^-23
#             relative.  sqrtf halves that, the reciprocal keeps it: the scale, and with it every result, is perturbed by at most 2^-23 relative = 2 ulps.
#   exp       device expf differs from libm's in the last place (csrc/ops.hip: ~2.5 % of arguments): 1 ulp.
#   sigmoid / silu / swiglu   e moves by one ulp, <= 2^-23 relative; 1 + e by e / (1 + e) of that, the quotient (and its product with b) likewise: 2 ulps.
#   tanh      one call of device tanhf against libm's.  No accuracy table of the device library ships with the toolchain; the bound taken is the one the
#             library is written to, OpenCL's full profile (tanh <= 5 ulp; sin, cos <= 4 ulp; log <= 3 ulp; pow <= 16 ulp).
#   soft_max  p = e * inv: e by one ulp of expf (2^-23 relative), inv through the sum of such values by at most as much: 2 * 2^-23 of p, hence of the
#             row's maximum.  With ALiBi the slope is one device powf (16 ulp = 2^-20 relative): the logit moves by 2^-20 * |slope * mask| and p by that
#             fraction — soft_max_alibi, which the case multiplies by ITS largest finite |slope * mask|.
#   rope      cos and sin by 4 ulp each, 4 * 2^-23 of mscale, times |x0| and |x1|: 8 * 2^-23 * mscale of the row's largest |x|.  YaRN's magnitude scale
#             1 + 0.1 logf(1 / freq_scale) holds one device logf (3 ulp of a term that is under an eighth of the sum): one more 2^-23.  For f16 data the
#             same: the final f16 rounding is in the baseline.
ALLOWANCE = {"rms_norm": 2.0, "exp": 1.0, "sigmoid": 2.0, "silu": 2.0, "swiglu": 2.0, "tanh": 5.0,
             "soft_max": 2 * 2.0 ** -23, "soft_max_alibi": 2.0 ** -20, "rope": 8 * 2.0 ** -23, "rope_f16": 8 * 2.0 ** -23, "rope_yarn": 9 * 2.0 ** -23}


# ------------------------------------------------------------------------------------------------ the cases (shared by the CPU and the GPU file)
class Case:
    """One small graph.  build(g) -> (outs, reads): the graph's output tensors and the tensors to read back after it ran (outputs, or the
    leaf a view writes into — read whole, so untouched bytes are checked against their sentinel).  expect() -> one array per read: f32 / f16 /
    integer for metric "bits", float64 for "ulp" (f32 ulps) and "row" (a fraction of the row's largest magnitude, or of `scale`)."""

    def __init__(self, cid, family, build, expect, metric="bits", extra=0.0, scale=None):
        self.id, self.family, self.build, self.expect, self.metric, self.extra, self.scale = cid, family, build, expect, metric, extra, scale

    def __repr__(self):
        return self.id


def run(case, target):
    """The case's graph on `target` ("oracle" or a Backend) -> the arrays of its reads."""
    import harness as T
    g = T.G(target)
    try:
        outs, reads = case.build(g)
        g.compute(list(outs))
        return [g.read(t) for t in reads]
    finally:
        g.free()


def distance(case, got, ref):
    """Largest distance of one read from the twin under the case's metric."""
    if case.metric == "ulp":
        return float(np.max(ulp_distance(got, ref)))
    return float(np.max(row_distance(got, ref, case.scale)))


@functools.lru_cache(maxsize=None)
def oracle_baseline(family):
    """The ORACLE's largest distance from the float64 twin over every case of a family: what the GPU gates start from."""
    worst = 0.0
    for c in all_cases():
        if c.family == family and c.metric != "bits":
            worst = max([worst] + [distance(c, g, r) for g, r in zip(run(c, "oracle"), c.expect())])
    return worst


def gate(case):
    """baseline + the family's allowance (+ the case's own term: ALiBi's slope error scales with the case's mask values)."""
    fam = case.family
    return oracle_baseline(fam) + ALLOWANCE[fam] + case.extra


def _as_view(r, root, nb, offs):
    """Turn the freshly built op node r into a view of the leaf `root` (strides nb, byte offset offs): the op then writes into root's memory,
    as an in-place op (ggml_*_inplace) or an op whose result the allocator placed inside another tensor does."""
    r.contents.view_src = root
    r.contents.view_offs = offs
    for i in range(4):
        r.contents.nb[i] = nb[i]
    return r


def _values(rng, n):
    """catalogue, then seeded values spanning +-100, n in all."""
    cat = catalogue()
    return np.concatenate([cat, seeded(rng, n - len(cat))])


def unary_cases():
    out = []
    for name in ("SILU", "RELU", "NEG", "EXP", "TANH", "SIGMOID"):
        x = _values(np.random.default_rng(100 + UNARY[name]), STRIDE_N)

        def build(g, x=x, name=name):
            r = g.H.ggml_unary(g.ctx, g.new(L.F32, [STRIDE_N], x), UNARY[name])
            return [r], [r]

        bitsop = name in UNARY_BITS
        out.append(Case(f"unary-{name}", name.lower(), build, lambda x=x, name=name: [unary(name, x).reshape(1, 1, 1, -1)], "bits" if bitsop else "ulp"))
    x = _values(np.random.default_rng(99), STRIDE_N)

    def build_inplace(g, x=x):  # ggml_neg_inplace: every element is read and written by exactly one thread
        a = g.new(L.F32, [STRIDE_N], x)
        r = _as_view(g.H.ggml_unary(g.ctx, a, UNARY["NEG"]), a, [4, 4 * STRIDE_N, 4 * STRIDE_N, 4 * STRIDE_N], 0)
        return [r], [r]

    out.append(Case("unary-NEG-inplace", "neg", build_inplace, lambda x=x: [unary("NEG", x).reshape(1, 1, 1, -1)]))
    return out


def scale_clamp_cases():
    out = []
    x = _values(np.random.default_rng(201), STRIDE_N)

    def build_scale(g):
        r = g.H.ggml_scale_bias(g.ctx, g.new(L.F32, [STRIDE_N], x), 0.37, -1.25)
        return [r], [r]

    out.append(Case("scale-stride", "scale", build_scale, lambda: [scale(x, 0.37, -1.25).reshape(1, 1, 1, -1)]))
    xs = _values(np.random.default_rng(202), 1000)

    def build_scale_big(g):
        r = g.H.ggml_scale_bias(g.ctx, g.new(L.F32, [250, 4], xs), 3e38, 65504.0)
        return [r], [r]

    out.append(Case("scale-overflow", "scale", build_scale_big, lambda: [scale(xs, 3e38, 65504.0).reshape(1, 1, 4, 250)]))
    for cid, n, lo, hi in (("clamp-stride", STRIDE_N, -1.5, 2.25), ("clamp-open-top", 1000, 6.103515625e-5, float("inf")), ("clamp-subnormal", 1000, -1e-40, 1e-41)):
        xc = _values(np.random.default_rng(203 + n % 7), n)

        def build(g, xc=xc, n=n, lo=lo, hi=hi):
            r = g.H.ggml_clamp(g.ctx, g.new(L.F32, [n], xc), lo, hi)
            return [r], [r]

        out.append(Case(cid, "clamp", build, lambda xc=xc, lo=lo, hi=hi: [clamp(xc, lo, hi).reshape(1, 1, 1, -1)]))
    return out


def cpy_cases():
    out = []
    rng = np.random.default_rng(301)
    cat = catalogue()
    x = np.concatenate([cat, seeded(rng, 4096), seeded(rng, 4096) * f32(700.0), seeded(rng, CPY_STRIDE_N - len(cat) - 8192 - 4096) * f32(1e-3),
                        (rng.integers(0, 0x7F800000, 4096, dtype=np.int64).astype(np.uint32) | (rng.integers(0, 2, 4096).astype(np.uint32) << 31)).view(np.float32)])

    def build_f32_f16(g):
        r = g.H.ggml_cast(g.ctx, g.new(L.F32, [CPY_STRIDE_N], x), L.F16)
        return [r], [r]

    out.append(Case("cpy-f32-f16-stride", "cpy", build_f32_f16, lambda: [cast(x, np.float16).reshape(1, 1, 1, -1)]))
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)  # every f16 there is

    def build_f16_f32(g):
        r = g.H.ggml_cast(g.ctx, g.new(L.F16, [256, 256], h), L.F32)
        return [r], [r]

    out.append(Case("cpy-f16-f32-all", "cpy", build_f16_f32, lambda: [cast(h, np.float32).reshape(1, 1, 256, 256)]))
    for cid, qt, dt, ax in (("cpy-i32-permuted", L.I32, np.int32, (0, 2, 1, 3)), ("cpy-f16-permuted", L.F16, np.float16, (1, 0, 2, 3)), ("cpy-f32-permuted", L.F32, np.float32, (2, 0, 3, 1))):
        if dt == np.int32:
            v = rng.integers(-2 ** 31, 2 ** 31 - 1, (2, 4, 3, 37), dtype=np.int64).astype(np.int32)
        else:
            v = cast(np.resize(np.concatenate([cat, seeded(rng, 500)]), (2, 4, 3, 37)), dt)

        def build(g, v=v, qt=qt, ax=ax):
            r = g.H.ggml_cont(g.ctx, g.H.ggml_permute(g.ctx, g.new(qt, [37, 3, 4, 2], v), *ax))
            return [r], [r]

        out.append(Case(cid, "cpy", build, lambda v=v, ax=ax, dt=dt: [cpy(permute(v, ax), dt)]))
    xs = np.concatenate([cat, seeded(rng, 3 * 4 * 37 - len(cat))]).reshape(1, 3, 4, 37)

    def build_f32_f16_strided(g):  # conversion through a transposed source
        r = g.H.ggml_cast(g.ctx, g.H.ggml_permute(g.ctx, g.new(L.F32, [37, 4, 3], xs), 1, 0, 2, 3), L.F16)
        return [r], [r]

    out.append(Case("cpy-f32-f16-transposed", "cpy", build_f32_f16_strided, lambda: [cpy(permute(xs, (1, 0, 2, 3)), np.float16)]))
    return out


def rms_norm_cases():
    out = []
    eps = 1e-5
    for ne0 in RMS_NE0:
        rng = np.random.default_rng(400 + ne0)
        x = (rng.standard_normal((3, ne0)) * rng.uniform(0.5, 30.0, (3, 1))).astype(np.float32)
        w = rng.uniform(0.5, 1.5, ne0).astype(np.float32)

        def build(g, x=x, w=w, ne0=ne0):
            H = g.H
            tx = g.new(L.F32, [ne0, 3], x)
            plain = H.ggml_rms_norm(g.ctx, tx, eps)
            fused = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, tx, eps), g.new(L.F32, [ne0], w))
            return [plain, fused], [plain, fused]

        out.append(Case(f"rms_norm-{ne0}", "rms_norm", build, lambda x=x, w=w: [rms_norm(x, eps).reshape((1, 1) + x.shape), rms_norm(x, eps, w).reshape((1, 1) + x.shape)], "ulp"))
    # special rows, on the scalar (100) and the vector path with a partial second trip (4100)
    for ne0 in (100, 4100):
        rng = np.random.default_rng(450 + ne0)
        x = np.zeros((5, ne0), np.float32)
        x[1] = f32(1e20) * rng.choice([-1.0, 1.0], ne0).astype(np.float32)
        x[2] = rng.integers(-100, 101, ne0).astype(np.float32) * f32(1e-41)
        x[3] = (rng.standard_normal(ne0) * 2).astype(np.float32)
        x[4] = 0.0
        x[4, ne0 - 1] = -3.0
        w = rng.uniform(0.5, 1.5, ne0).astype(np.float32)

        def build(g, x=x, w=w, ne0=ne0):
            H = g.H
            tx = g.new(L.F32, [ne0, 5], x)
            plain = H.ggml_rms_norm(g.ctx, tx, eps)
            fused = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, tx, eps), g.new(L.F32, [ne0], w))
            return [plain, fused], [plain, fused]

        out.append(Case(f"rms_norm-special-rows-{ne0}", "rms_norm", build, lambda x=x, w=w: [rms_norm(x, eps).reshape((1, 1) + x.shape), rms_norm(x, eps, w).reshape((1, 1) + x.shape)], "ulp"))
    # row views of a wider tensor: at a 4-byte offset (rows off 16-byte alignment: the scalar path although ne0 % 4 == 0) and padded rows that stay aligned
    for cid, ne0, pad, off in (("rms_norm-view-offset4", 4100, 4, 1), ("rms_norm-view-padded", 4096, 8, 0), ("rms_norm-view-padded-tail", 4100, 4, 0)):
        rng = np.random.default_rng(470 + ne0 + off)
        base = (rng.standard_normal((3, ne0 + pad)) * 5).astype(np.float32)
        base[:, ne0 + off:] = 1000.0  # what lies behind a row is not part of it
        base[:, :off] = -1000.0
        w = rng.uniform(0.5, 1.5, ne0).astype(np.float32)

        def build(g, base=base, w=w, ne0=ne0, pad=pad, off=off):
            H = g.H
            v = H.ggml_view_2d(g.ctx, g.new(L.F32, [ne0 + pad, 3], base), ne0, 3, (ne0 + pad) * 4, off * 4)
            plain = H.ggml_rms_norm(g.ctx, v, eps)
            fused = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, v, eps), g.new(L.F32, [ne0], w))
            return [plain, fused], [plain, fused]

        def expect(base=base, w=w, ne0=ne0, off=off):
            x = base[:, off:off + ne0]
            return [rms_norm(x, eps).reshape(1, 1, 3, ne0), rms_norm(x, eps, w).reshape(1, 1, 3, ne0)]

        out.append(Case(cid, "rms_norm", build, expect, "ulp"))
    return out


def swiglu_cases():
    """The gate operand takes the whole catalogue; the multiplier only its exact values (0, +-1, 0.5, +-inf, NaN) among Gaussian ones: a subnormal silu times a
    large multiplier would turn f32's absolute 2^-149 grid into a relative error of the product — the definition's own, not an implementation's."""
    out = []
    cat = catalogue()
    exact = np.array([0.0, -0.0, 1.0, -1.0, 0.5, np.inf, -np.inf, np.nan], np.float32)
    for nc in GLU_NC:
        rng = np.random.default_rng(500 + nc)
        a = np.resize(np.concatenate([cat, seeded(rng, 3 * nc)]), (3, nc)).astype(np.float32)
        b = (rng.standard_normal((3, nc)) * 2).astype(np.float32)
        b[1, :: 5] = np.resize(exact, len(b[1, :: 5]))

        def build(g, a=a, b=b, nc=nc):
            r = g.H.ggml_swiglu_split(g.ctx, g.new(L.F32, [nc, 3], a), g.new(L.F32, [nc, 3], b))
            return [r], [r]

        out.append(Case(f"swiglu-split-{nc}", "swiglu", build, lambda a=a, b=b: [swiglu(a, b).reshape((1, 1) + a.shape)], "ulp"))
        for swapped in (0, 1):
            x = np.concatenate([b, a] if swapped else [a, b], axis=1)  # swapped: the gate is the SECOND half of the row

            def build_h(g, x=x, nc=nc, swapped=swapped):
                r = g.H.ggml_swiglu(g.ctx, g.new(L.F32, [2 * nc, 3], x))
                r.contents.op_params[1] = swapped  # ggml_swiglu_swapped
                return [r], [r]

            out.append(Case(f"swiglu-halves-{nc}-swapped{swapped}", "swiglu", build_h, lambda a=a, b=b: [swiglu(a, b).reshape((1, 1) + a.shape)], "ulp"))
    return out


def _mask(rng, shape, np_dtype):
    m = np.where(rng.uniform(size=shape) < 0.3, -np.inf, 0.0).astype(np.float32)
    m[..., 0] = 0.0
    m = m + np.where(np.isfinite(m), rng.integers(-3, 1, shape).astype(np.float32), f32(0.0))
    return m.astype(np_dtype)


def soft_max_cases():
    out = []
    MT = {L.F16: np.float16, L.F32: np.float32}
    for k, n in enumerate(SOFTMAX_N):
        rng = np.random.default_rng(600 + n)
        heads, rows = 3, 2
        x = (rng.standard_normal((1, heads, rows, n)) * 5).astype(np.float32)
        mt = (L.F16, L.F32, None)[k % 3]  # (8193, the one size on the generic k_soft_max, gets an F16 mask)
        m = None if mt is None else _mask(rng, (1, 1, rows + 1, n), MT[mt])

        def build(g, x=x, m=m, mt=mt, n=n, heads=heads, rows=rows):
            tm = None if mt is None else g.new(mt, [n, rows + 1], m)
            r = g.H.ggml_soft_max_ext(g.ctx, g.new(L.F32, [n, rows, heads], x), tm, 0.125, 0.0)
            return [r], [r]

        out.append(Case(f"soft_max-n{n}-mask{mt}", "soft_max", build, lambda x=x, m=m: [soft_max(x, m, 0.125)], "row"))
    # batch dimension; masks that broadcast over heads and batch with 1 < mask.ne[2] < heads and 1 < mask.ne[3] < ne[3]
    for cid, xs, ms, mt in (("soft_max-ne3-mask-1-1", (2, 3, 2, 1025), (1, 1, 2, 1025), L.F16), ("soft_max-mask-ne2-ne3", (4, 4, 2, 33), (2, 2, 2, 33), L.F32),
                            ("soft_max-mask-heads-batch", (2, 3, 2, 257), (2, 3, 2, 257), L.F16)):
        rng = np.random.default_rng(650 + xs[0] + xs[3])
        x = (rng.standard_normal(xs) * 5).astype(np.float32)
        m = _mask(rng, ms, MT[mt])

        def build(g, x=x, m=m, mt=mt, xs=xs, ms=ms):
            r = g.H.ggml_soft_max_ext(g.ctx, g.new(L.F32, list(xs[::-1]), x), g.new(mt, list(ms[::-1]), m), 0.25, 0.0)
            return [r], [r]

        out.append(Case(cid, "soft_max", build, lambda x=x, m=m: [soft_max(x, m, 0.25)], "row"))
    # an f16 mask whose rows are a padded view
    rng = np.random.default_rng(660)
    n, pad = 1025, 7
    xv = (rng.standard_normal((1, 2, 3, n)) * 5).astype(np.float32)
    mb = _mask(rng, (3, n + pad), np.float16)
    mb[:, n:] = np.float16(-7.0)

    def build_view(g):
        tm = g.H.ggml_view_2d(g.ctx, g.new(L.F16, [n + pad, 3], mb), n, 3, (n + pad) * 2, 0)
        r = g.H.ggml_soft_max_ext(g.ctx, g.new(L.F32, [n, 3, 2], xv), tm, 0.125, 0.0)
        return [r], [r]

    out.append(Case("soft_max-mask-padded-view", "soft_max", build_view, lambda: [soft_max(xv, mb[:, :n], 0.125)], "row"))
    # the generic k_soft_max (rows above the register kernels' 8192): a mask that repeats over the heads (1 < mask.ne[2] < heads), its rows a padded view
    rng = np.random.default_rng(665)
    ng, padg = 8200, 8
    xg = (rng.standard_normal((1, 4, 2, ng)) * 5).astype(np.float32)
    mg = _mask(rng, (2, 2, ng + padg), np.float16)
    mg[..., ng:] = np.float16(-7.0)

    def build_generic(g):
        tm = g.H.ggml_view_3d(g.ctx, g.new(L.F16, [ng + padg, 2, 2], mg), ng, 2, 2, (ng + padg) * 2, (ng + padg) * 2 * 2, 0)
        r = g.H.ggml_soft_max_ext(g.ctx, g.new(L.F32, [ng, 2, 4], xg), tm, 0.125, 0.0)
        return [r], [r]

    out.append(Case("soft_max-generic-mask-mod-padded", "soft_max", build_generic, lambda: [soft_max(xg, mg[None, :, :, :ng], 0.125)], "row"))
    # ALiBi on six heads (slopes change formula at head 4)
    rng = np.random.default_rng(670)
    xa = (rng.standard_normal((1, 6, 2, 100)) * 5).astype(np.float32)
    ma = -np.abs(np.arange(100)[None, :] - np.array([[99], [50]])).astype(np.float32)
    ma[:, 7] = -np.inf
    ma = ma.astype(np.float16)

    def build_alibi(g):
        r = g.H.ggml_soft_max_ext(g.ctx, g.new(L.F32, [100, 2, 6], xa), g.new(L.F16, [100, 2], ma), 0.125, 8.0)
        return [r], [r]

    out.append(Case("soft_max-alibi-6-heads", "soft_max", build_alibi, lambda: [soft_max(xa, ma, 0.125, 8.0)], "row", extra=ALLOWANCE["soft_max_alibi"] * float(np.max(alibi_slopes(6, 8.0)) * 99.0)))  # largest finite |slope * mask|: head 4's slope, 0.5, at distance 99
    # sinks, and a fully masked row (the zero-sum guard)
    rng = np.random.default_rng(680)
    xk = rng.standard_normal((1, 4, 2, 1025)).astype(np.float32)
    sk = (rng.standard_normal(4) * 3).astype(np.float32)
    mk = np.zeros((2, 1025), np.float32)
    mk[1, :] = -np.inf

    def build_sinks(g, with_sinks=True):
        r = g.H.ggml_soft_max_ext(g.ctx, g.new(L.F32, [1025, 2, 4], xk), g.new(L.F32, [1025, 2], mk), 1.0, 0.0)
        if with_sinks:
            g.H.ggml_soft_max_add_sinks(r, g.new(L.F32, [4], sk))
        return [r], [r]

    out.append(Case("soft_max-sinks", "soft_max", build_sinks, lambda: [soft_max(xk, mk, 1.0, 0.0, sk)], "row", scale=np.ones((1, 4, 2))))
    out.append(Case("soft_max-fully-masked-row", "soft_max", lambda g: build_sinks(g, False), lambda: [soft_max(xk, mk, 1.0)], "row"))
    return out


def argmax_cases():
    out = []
    for n in (1, 63, 65, 255, 257, 1025):
        rng = np.random.default_rng(700 + n)
        rows = [rng.standard_normal(n), -np.abs(rng.standard_normal(n)) - 1.0, np.full(n, -np.inf)]
        r = rng.standard_normal(n)  # NaN in front of and behind the maximum
        r[n // 2] = 50.0
        r[0] = np.nan
        if n > 2:
            r[n - 1] = np.nan
        rows.append(r)
        rows.append(np.full(n, np.nan))

        def tie(i, j):
            t = rng.standard_normal(n)
            t[i] = t[j] = 99.0
            rows.append(t)

        if n > 1:
            tie(n - 2, n - 1)            # neighbouring lanes
        if n > 40:
            tie(40, 3)                   # two lanes of one wave
        if n > 70:
            tie(5, 70)                   # two waves, the first index in the lower wave
        if n > 256:
            tie(0, 256)                  # one thread's stride
            tie(10, 256)                 # a thread's SECOND element against another lane's first: meets in the butterfly
        if n > 300:
            tie(100, 300)                # the first index sits in the HIGHER wave (thread 100 against thread 44): the cross-wave step decides
            tie(300, 600)
            t = np.full(n, -np.inf)      # -inf everywhere but late in the row
            t[1000] = -1e30
            rows.append(t)
        x = np.stack(rows).astype(np.float32)

        def build(g, x=x, n=n):
            r = g.H.ggml_argmax(g.ctx, g.new(L.F32, [n, x.shape[0]], x))
            return [r], [r]

        out.append(Case(f"argmax-{n}", "argmax", build, lambda x=x: [argmax(x).reshape(1, 1, 1, -1)]))
    return out


def get_rows_cases():
    out = []
    for qt, dt in ((L.F32, np.float32), (L.F16, np.float16)):
        for ne0 in (1, 40, 1030):
            rng = np.random.default_rng(800 + ne0 + qt)
            a = (rng.standard_normal((2, 3, 7, ne0)) * 10).astype(dt)
            a[0, 0, 0, :] = cast(np.resize(catalogue(), ne0), dt)
            idx3 = rng.integers(0, 7, (2, 3, 5)).astype(np.int32)
            idx3[0, 0] = [0, 6, 3, 3, 0]  # repeated indices
            idx2 = np.ascontiguousarray(idx3[1])

            def build3(g, a=a, idx3=idx3, qt=qt, ne0=ne0):
                r = g.H.ggml_get_rows(g.ctx, g.new(qt, [ne0, 7, 3, 2], a), g.new(L.I32, [5, 3, 2], idx3))
                return [r], [r]

            def build2(g, a=a, idx2=idx2, qt=qt, ne0=ne0):
                r = g.H.ggml_get_rows(g.ctx, g.new(qt, [ne0, 7, 3], a[1]), g.new(L.I32, [5, 3], idx2))
                return [r], [r]

            out.append(Case(f"get_rows-{L.TYPE_NAME[qt]}-{ne0}-idx3d", "get_rows", build3, lambda a=a, idx3=idx3: [get_rows(a, idx3)]))
            out.append(Case(f"get_rows-{L.TYPE_NAME[qt]}-{ne0}-idx2d", "get_rows", build2, lambda a=a, idx2=idx2: [get_rows(a[1], idx2).reshape(1, 3, 5, -1)]))
    return out


def _sentinel(shape, dt):
    s = (np.arange(int(np.prod(shape))) % 251 + 1000).reshape(shape)
    return s.astype(dt)


def set_rows_cases():
    out = []
    cat = catalogue()
    for qt, dt in ((L.F32, np.float32), (L.F16, np.float16)):
        es = np.dtype(dt).itemsize
        for nc in SET_ROWS_NC:
            rng = np.random.default_rng(900 + nc + qt)
            src = np.resize(np.concatenate([cat, seeded(rng, 7 * nc) * f32(50.0)]), (7, nc)).astype(np.float32)
            idx = np.array([3, 0, 19, 5, 6, 31, 12], np.int64)
            base = _sentinel((32, nc), dt)

            def build(g, src=src, idx=idx, base=base, qt=qt, nc=nc):
                r = g.H.ggml_set_rows(g.ctx, g.new(qt, [nc, 32], base), g.new(L.F32, [nc, 7], src), g.new(L.I64, [7], idx))
                return [r], [r]

            out.append(Case(f"set_rows-{L.TYPE_NAME[qt]}-{nc}", "set_rows", build, lambda src=src, idx=idx, base=base: [set_rows(base, src, idx).reshape((1, 1) + base.shape)]))
        # destination rows one element into a wider tensor: off 16-byte alignment, so the scalar path although nc % 4 == 0; the whole leaf is read back
        nc, wide = 256, 260
        rng = np.random.default_rng(950 + qt)
        src = (seeded(rng, 7 * nc) * f32(50.0)).reshape(7, nc)
        idx = np.array([3, 0, 19, 5, 6, 31, 12], np.int64)
        base = _sentinel((32, wide), dt)

        def build_view(g, src=src, idx=idx, base=base, qt=qt, es=es):
            leaf = g.new(qt, [wide, 32], base)
            v = g.H.ggml_view_2d(g.ctx, leaf, nc, 32, wide * es, es)
            r = g.H.ggml_set_rows(g.ctx, v, g.new(L.F32, [nc, 7], src), g.new(L.I64, [7], idx))
            return [r], [leaf]

        def expect_view(src=src, idx=idx, base=base):
            e = base.copy()
            e[:, 1:1 + nc] = set_rows(base[:, 1:1 + nc], src, idx)
            return [e.reshape(1, 1, 32, wide)]

        out.append(Case(f"set_rows-{L.TYPE_NAME[qt]}-misaligned-view", "set_rows", build_view, expect_view))
        # 3-D sources: the index tensor broadcast over the heads (idx.ne[1] = 1), and 1 < idx.ne[1] < ne2
        for cid, n2, i1 in ((f"set_rows-{L.TYPE_NAME[qt]}-3d-broadcast", 3, 1), (f"set_rows-{L.TYPE_NAME[qt]}-3d-idx-mod", 4, 2)):
            rng = np.random.default_rng(960 + qt + n2)
            src3 = (seeded(rng, n2 * 5 * nc) * f32(50.0)).reshape(1, n2, 5, nc)
            idxb = np.stack([rng.permutation(16)[:5] for _ in range(i1)]).astype(np.int64).reshape(1, i1, 5)
            base3 = _sentinel((1, n2, 16, nc), dt)

            def build3(g, src3=src3, idxb=idxb, base3=base3, qt=qt, n2=n2, i1=i1):
                r = g.H.ggml_set_rows(g.ctx, g.new(qt, [nc, 16, n2], base3), g.new(L.F32, [nc, 5, n2], src3), g.new(L.I64, [5, i1], idxb))
                return [r], [r]

            out.append(Case(cid, "set_rows", build3, lambda src3=src3, idxb=idxb, base3=base3: [set_rows(base3, src3, idxb)]))
        # element scatter (rows of one value: a transposed V cache) from a 3-D source
        rng = np.random.default_rng(980 + qt)
        vals = (seeded(rng, 3 * 40) * f32(50.0)).reshape(1, 3, 40, 1)
        eidx = np.stack([rng.permutation(512)[:40] for _ in range(3)]).astype(np.int64).reshape(1, 3, 40)
        ebase = _sentinel((1, 3, 512, 1), dt)

        def build_e(g, vals=vals, eidx=eidx, ebase=ebase, qt=qt):
            r = g.H.ggml_set_rows(g.ctx, g.new(qt, [1, 512, 3], ebase), g.new(L.F32, [1, 40, 3], vals), g.new(L.I64, [40, 3], eidx))
            return [r], [r]

        out.append(Case(f"set_rows-{L.TYPE_NAME[qt]}-element-scatter-3d", "set_rows", build_e, lambda vals=vals, eidx=eidx, ebase=ebase: [set_rows(ebase, vals, eidx)]))
    return out


ROPE_POS = np.array([0, 1, 131071, 1000000], np.int32)


def rope_cases():
    out = []
    for neox in (0, 1):
        for HD in (2, 64, 256):
            for n_dims in sorted({2, HD // 2, HD} - {1}):
                rng = np.random.default_rng(1000 + HD + n_dims + neox)
                x = (rng.standard_normal((2, 4, 2, HD)) * 3).astype(np.float32)
                base = 10000.0 if HD == 64 else 500000.0

                def build(g, x=x, HD=HD, n_dims=n_dims, neox=neox, base=base):
                    r = g.H.ggml_rope_ext(g.ctx, g.new(L.F32, [HD, 2, 4, 2], x), g.new(L.I32, [4], ROPE_POS), None, n_dims, L.ROPE_NEOX if neox else 0, 8192, base, 1.0, 0.0, 1.0, 32.0, 1.0)
                    return [r], [r]

                out.append(Case(f"rope-{'neox' if neox else 'normal'}-hd{HD}-nd{n_dims}", "rope", build, lambda x=x, n_dims=n_dims, neox=neox, base=base: [rope(x, ROPE_POS, n_dims, neox, base)],
                                "row", scale=np.max(np.abs(x), axis=-1)))
    # the q slice of a wider (fused q | k | v) tensor: rows contiguous, heads and tokens strided
    rng = np.random.default_rng(1100)
    HD, NH = 64, 3
    wide = (rng.standard_normal((4, 3 * NH * HD)) * 3).astype(np.float32)

    def build_slice(g, neox):
        v = g.H.ggml_view_3d(g.ctx, g.new(L.F32, [3 * NH * HD, 4], wide), HD, NH, 4, HD * 4, 3 * NH * HD * 4, NH * HD * 4)
        r = g.H.ggml_rope_ext(g.ctx, v, g.new(L.I32, [4], ROPE_POS), None, HD, L.ROPE_NEOX if neox else 0, 8192, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        return [r], [r]

    ks = wide[:, NH * HD:2 * NH * HD].reshape(1, 4, NH, HD)
    for neox in (0, 1):
        out.append(Case(f"rope-strided-slice-{'neox' if neox else 'normal'}", "rope", lambda g, neox=neox: build_slice(g, neox), lambda neox=neox: [rope(ks, ROPE_POS, HD, neox, 10000.0)],
                        "row", scale=np.max(np.abs(ks), axis=-1)))
    # frequency factors + YaRN over 128 pairs (the lane loop's second trip reads ff[64 ..])
    rng = np.random.default_rng(1110)
    xy = (rng.standard_normal((1, 4, 2, 256)) * 3).astype(np.float32)
    ffv = rng.uniform(1.0, 8.0, 128).astype(np.float32)

    def build_yarn(g):
        r = g.H.ggml_rope_ext(g.ctx, g.new(L.F32, [256, 2, 4], xy), g.new(L.I32, [4], ROPE_POS), g.new(L.F32, [128], ffv), 256, L.ROPE_NEOX, 8192, 500000.0, 0.25, 1.0, 1.1, 32.0, 1.0)
        return [r], [r]

    msc = 1.1 * (1.0 + 0.1 * np.log(4.0))
    out.append(Case("rope-yarn-ff-hd256", "rope_yarn", build_yarn, lambda: [rope(xy, ROPE_POS, 256, 1, 500000.0, 0.25, 1.0, 1.1, ff=ffv)], "row", scale=np.max(np.abs(xy), axis=-1) * msc))
    # f16 data with a pass-through tail; the in-place K-shift form with negative shifts
    rng = np.random.default_rng(1120)
    xh = (rng.standard_normal((1, 4, 2, 64)) * 3).astype(np.float16)
    shift = np.array([-3, -1000, 7, 0], np.int32)
    for cid, neox, inplace, pos, nd in (("rope-f16-tail-normal", 0, False, ROPE_POS, 32), ("rope-f16-tail-neox", 1, False, ROPE_POS, 32), ("rope-f16-kshift-inplace", 0, True, shift, 64),
                                        ("rope-f16-kshift-inplace-neox", 1, True, shift, 64)):
        def build_h(g, neox=neox, inplace=inplace, pos=pos, nd=nd):
            fn = g.H.ggml_rope_ext_inplace if inplace else g.H.ggml_rope_ext
            r = fn(g.ctx, g.new(L.F16, [64, 2, 4], xh), g.new(L.I32, [4], pos), None, nd, L.ROPE_NEOX if neox else 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
            return [r], [r]

        out.append(Case(cid, "rope_f16", build_h, lambda neox=neox, pos=pos, nd=nd: [rope(xh, pos, nd, neox, 500000.0)], "row", scale=np.max(np.abs(xh.astype(np.float64)), axis=-1)))
    xi = (rng.standard_normal((1, 4, 2, 64)) * 3).astype(np.float32)

    def build_inplace(g):
        r = g.H.ggml_rope_ext_inplace(g.ctx, g.new(L.F32, [64, 2, 4], xi), g.new(L.I32, [4], shift), None, 64, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        return [r], [r]

    out.append(Case("rope-f32-kshift-inplace", "rope", build_inplace, lambda: [rope(xi, shift, 64, 0, 500000.0)], "row", scale=np.max(np.abs(xi), axis=-1)))
    return out


def binary_cases():
    out = []
    cat = catalogue()
    nc = len(cat)
    for op in ("add", "sub", "mul", "div"):
        rng = np.random.default_rng(1200 + len(op) + ord(op[0]))
        A = rng.standard_normal((2, 3, 5, 64)).astype(np.float32)
        Bp = (rng.standard_normal((2, 5, 3, 64)) + 3.0).astype(np.float32)
        b16 = (rng.standard_normal(16) + 3.0).astype(np.float32)

        def build_perm(g, op=op, A=A, Bp=Bp):
            H = g.H
            a = H.ggml_permute(g.ctx, g.new(L.F32, [64, 5, 3, 2], A), 0, 2, 1, 3)
            r = getattr(H, "ggml_" + op)(g.ctx, a, g.new(L.F32, [64, 3, 5, 2], Bp))
            return [r], [r]

        out.append(Case(f"{op}-permuted-a", "binary", build_perm, lambda op=op, A=A, Bp=Bp: [binary(op, np.ascontiguousarray(permute(A, (0, 2, 1, 3))), Bp)]))

        def build_b16(g, op=op, A=A, b16=b16):
            H = g.H
            a = H.ggml_permute(g.ctx, g.new(L.F32, [64, 5, 3, 2], A), 0, 2, 1, 3)
            r = getattr(H, "ggml_" + op)(g.ctx, a, g.new(L.F32, [16], b16))
            return [r], [r]

        out.append(Case(f"{op}-b16-under-a64", "binary", build_b16, lambda op=op, A=A, b16=b16: [binary(op, np.ascontiguousarray(permute(A, (0, 2, 1, 3))), b16)]))
        big = _sentinel((2, 3, 5, 80), np.float32)

        def build_dst(g, op=op, A=A, Bp=Bp, big=big):  # the result lives inside a wider tensor: rows of 64 at element 8 of rows of 80
            H = g.H
            leaf = g.new(L.F32, [80, 5, 3, 2], big)
            r = getattr(H, "ggml_" + op)(g.ctx, g.new(L.F32, [64, 5, 3, 2], A), g.new(L.F32, [64, 5, 3, 1], np.ascontiguousarray(Bp.transpose(0, 2, 1, 3)[:1])))
            _as_view(r, leaf, [4, 80 * 4, 80 * 5 * 4, 80 * 5 * 3 * 4], 8 * 4)
            return [r], [leaf]

        def expect_dst(op=op, A=A, Bp=Bp, big=big):
            e = big.copy()
            e[..., 8:72] = binary(op, A, np.ascontiguousarray(Bp.transpose(0, 2, 1, 3)[:1]))
            return [e]

        out.append(Case(f"{op}-strided-destination", "binary", build_dst, expect_dst))
        a_cat = np.tile(cat, (nc, 1))          # a[j, i] = cat[i]
        b_cat = cat.reshape(nc, 1).copy()      # b[j] = cat[j], broadcast along the row: every pair of catalogue values — 0/0, x/0, inf - inf, subnormal products

        def build_cat(g, op=op):
            r = getattr(g.H, "ggml_" + op)(g.ctx, g.new(L.F32, [nc, nc], a_cat), g.new(L.F32, [1, nc], b_cat))
            return [r], [r]

        out.append(Case(f"{op}-catalogue-pairs", "binary", build_cat, lambda op=op: [binary(op, a_cat, b_cat).reshape(1, 1, nc, nc)]))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(unary_cases() + scale_clamp_cases() + cpy_cases() + rms_norm_cases() + swiglu_cases() + soft_max_cases() + argmax_cases() + get_rows_cases() + set_rows_cases() +
                 rope_cases() + binary_cases())
