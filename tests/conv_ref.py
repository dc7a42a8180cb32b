"""NumPy twins of the tower ops of csrc/conv.hip: IM2COL, MUL_MAT f16 x f16, POOL_2D / POOL_1D, PAD and UPSCALE.

No ggml source is at hand and the CPU oracle has none of these ops, so — as for Q2_K / Q3_K — nothing on record pins them: the contracts are restated from
ggml-cpu's behaviour at the ABI snapshot of include/ggml_abi.h, and the twins below ARE the reference the kernels are held to.  Every op has a
float64 twin (the mathematical value) and an f32 twin that performs the stated operations in the stated order in np.float32; the GPU is compared bit for bit with
the f32 twin wherever the contract fixes the order (everything but the mat-mul), and the f32 twins are held against the float64 twins within the bounds derived here.

Arrays are indexed as NumPy sees a contiguous ggml tensor: shape = ne reversed, so data [IW, IH, IC, N] is x[n, ic, ih, iw].

Bounds (u = 2^-24, the unit roundoff of f32; first order in u):
  im2col to f16:  one round-to-nearest-even of an f32: |err| <= 2^-11 |x| for normal results, 2^-25 absolute below the smallest normal f16.  To f32, PAD: exact.
  mul_mat:        products of two f16 values are exact in f32 (22 significant bits), so only the K - 1 additions round.  With partial sums behaving as a random
                  walk the error variance of a sequential f32 sum is about u^2 K / 6 of the result's variance (each addition rounds a partial sum of ~sqrt(k) terms by
                  a uniform error of variance (u s_k)^2 / 3): NMSE ~ 6e-16 K, 7e-13 at K = 1176.  The project's gate for this arithmetic is NMSE <= 1e-11
                  (tests/test_gpu_ops.py::test_mul_mat_f); it holds for K up to ~17 000 and is what both the f32 twin and the GPU are held to against float64.
  pool AVG:       n = k0 k1 cells: n - 1 additions and one division, each within u: |err| <= n u sum|v| / (k0 k1).  MAX: exact.
  upscale:        nearest is a gather whose index arithmetic is part of the contract (the float64 twin uses the same f32 quotient): exact.  Bilinear: the value is
                  continuous and piecewise linear in the sample position x, with slope at most 2 max|v| a pixel; x = (i + 0.5) / sf - 0.5 carries three roundings of
                  quantities no larger than W + 1, so |dx err| <= 3 (W + 1) u, likewise for y; the weights and the four products and three sums add at most 10 u max|v|.
                  |err| <= (6 (W + H + 2) + 10) u max|v| with W, H the SOURCE extents.
"""
import numpy as np

U = 2.0 ** -24
F16_MIN_NORMAL = 2.0 ** -14
MM_NMSE_GATE = 1e-11  # tests/test_gpu_ops.py::test_mul_mat_f


def out_extent(n, k, s, p, d):
    """(n + 2 p - d (k - 1) - 1) / s + 1"""
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


# ------------------------------------------------------------------------------------------------ IM2COL
def im2col(x, KH, KW, s0, s1, p0, p1, d0, d1, dtype, wrong=None):
    """x [N, IC, IH, IW] -> [N, OH, OW, IC * KH * KW] of `dtype`:
    dst[n, oh, ow, ic * KH * KW + kh * KW + kw] = x[n, ic, oh * s1 + kh * d1 - p1, ow * s0 + kw * d0 - p0], zero outside the image, rounded to nearest even when
    dtype is np.float16.  dtype np.float64 is the float64 twin: the same gather, unrounded.  The 1-D form is KH = IH = 1, s1 = d1 = 1, p1 = 0.
    wrong: "swap_khkw" indexes the column as kw * KH + kh; "no_dilation" reads with d0 = d1 = 1 (the result's extents still follow the real dilation)."""
    N, IC, IH, IW = x.shape
    OH, OW = out_extent(IH, KH, s1, p1, d1), out_extent(IW, KW, s0, p0, d0)
    out = np.zeros((N, OH, OW, IC * KH * KW), dtype=np.float64)
    e0, e1 = (1, 1) if wrong == "no_dilation" else (d0, d1)
    oh, ow = np.arange(OH)[:, None], np.arange(OW)[None, :]
    for ic in range(IC):
        for kh in range(KH):
            for kw in range(KW):
                ih, iw = oh * s1 + kh * e1 - p1, ow * s0 + kw * e0 - p0
                ok = (ih >= 0) & (ih < IH) & (iw >= 0) & (iw < IW)
                v = x[:, ic][:, np.clip(ih, 0, IH - 1), np.clip(iw, 0, IW - 1)].astype(np.float64)
                col = ic * KH * KW + (kw * KH + kh if wrong == "swap_khkw" else kh * KW + kw)
                out[:, :, :, col] = np.where(ok[None], v, 0.0)
    return out.astype(dtype)


def im2col_gate(want64, dtype):
    """The bound on |f16 or f32 result - float64 twin| per element."""
    if dtype != np.float16:
        return np.zeros_like(want64)
    return np.maximum(2.0 ** -11 * np.abs(want64), 2.0 ** -25)


# ------------------------------------------------------------------------------------------------ MUL_MAT f16 x f16
def _bcast(a, nb2, nb3):
    """src0 [A3, A2, Na, K] repeated over src1's batches [B3, B2]: batch (i3, i2) of src1 reads batch (i3 // (B3 / A3), i2 // (B2 / A2))."""
    return np.repeat(np.repeat(a, nb3 // a.shape[0], axis=0), nb2 // a.shape[1], axis=1)


def _as4(m):
    m = np.asarray(m)
    return m.reshape((1,) * (4 - m.ndim) + m.shape)


def mul_mat64(a, b):
    """a f16 [.., Na, K], b f16 [.., Nb, K] -> float64 [.., Nb, Na]: exact products of the f16 values, summed in float64 (ggml's result is ne [Na, Nb, ..])."""
    a, b = _as4(a), _as4(b)
    assert a.dtype == np.float16 and b.dtype == np.float16
    a = _bcast(a, b.shape[1], b.shape[0]).astype(np.float64)
    return np.einsum("...nk,...mk->...mn", a, b.astype(np.float64))


def mul_mat32(a, b, wrong=None):
    """The f32 twin: neither operand rounded, exact f32 products, summed in f32 in ascending k.  wrong: "round_bf16" first drops the operands' low 8 mantissa bits
    (a kernel that took the bf16 instruction)."""
    a, b = _as4(a), _as4(b)
    a = _bcast(a, b.shape[1], b.shape[0]).astype(np.float32)
    b = b.astype(np.float32)
    if wrong == "round_bf16":
        a, b = [(t.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32) for t in (a, b)]
    prod = b[..., :, None, :] * a[..., None, :, :]
    return np.add.accumulate(prod, axis=-1, dtype=np.float32)[..., -1]


def nmse(got, want):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    den = float(np.sum(want * want))
    num = float(np.sum((got - want) ** 2))
    return num / den if den else (0.0 if num == 0.0 else float("inf"))


# ------------------------------------------------------------------------------------------------ POOL_2D / POOL_1D
MAX, AVG = 0, 1


def pool2d(x, op, k0, k1, s0, s1, p0, p1, f=np.float32, wrong=None):
    """x [N3, N2, H, W] -> [N3, N2, (H + 2 p1 - k1) / s1 + 1, (W + 2 p0 - k0) / s0 + 1] in `f` (np.float32: the f32 twin, np.float64: the float64 twin).
    Each output starts at 0 (AVG) or -FLT_MAX (MAX), walks ky outer and kx inner from (ox s0 - p0, oy s1 - p1), skips cells outside the plane, accumulates in that
    order (MAX: the cell replaces the accumulator when it is greater); AVG then divides by (float) (k0 k1) — padding cells count in the divisor.
    wrong: "valid_divisor" divides by the number of cells inside the plane."""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    OH, OW = (H + 2 * p1 - k1) // s1 + 1, (W + 2 * p0 - k0) // s0 + 1
    oy, ox = np.arange(OH)[:, None], np.arange(OW)[None, :]
    acc = np.full(x.shape[:-2] + (OH, OW), 0.0 if op == AVG else -np.finfo(np.float32).max, dtype=f)
    cnt = np.zeros((OH, OW))
    for ky in range(k1):
        for kx in range(k0):
            y, xx = oy * s1 - p1 + ky, ox * s0 - p0 + kx
            ok = (y >= 0) & (y < H) & (xx >= 0) & (xx < W)
            ok, y, xx = np.broadcast_arrays(ok, y, xx)
            v = x[..., np.clip(y, 0, H - 1), np.clip(xx, 0, W - 1)].astype(f)
            if op == AVG:
                acc = np.where(ok, acc + v, acc)
            else:
                acc = np.where(ok & (v > acc), v, acc)
            cnt = cnt + ok
    if op == AVG:
        acc = acc / (np.maximum(cnt, 1).astype(f) if wrong == "valid_divisor" else f(k0 * k1))
    assert acc.dtype == f
    return acc


def pool1d(x, op, k0, f=np.float32):
    """x [.., W] -> [.., (W - k0) / k0 + 1]: the only form ggml-cpu computes, k0 == s0 and p0 == 0; the same accumulate-then-divide rule (a tail shorter than k0 is dropped)."""
    x = np.asarray(x)
    x4 = x.reshape((-1, 1, 1, x.shape[-1]))
    r = pool2d(x4, op, k0, 1, k0, 1, 0, 0, f)
    return r.reshape(x.shape[:-1] + (r.shape[-1],))


def pool_avg_gate(x, k0, k1, s0, s1, p0, p1):
    """n u sum|v| / (k0 k1) per output, n = k0 k1."""
    return k0 * k1 * U * pool2d(np.abs(np.asarray(x, dtype=np.float64)), AVG, k0, k1, s0, s1, p0, p1, np.float64) * 1.0000001


# ------------------------------------------------------------------------------------------------ PAD
def pad(x, ne):
    """x -> shape `ne` (NumPy order, every extent >= x's): x at the low indices, zero elsewhere.  Exact; the same array serves as both twins."""
    out = np.zeros(ne, dtype=x.dtype)
    out[tuple(slice(0, n) for n in x.shape)] = x
    return out


# ------------------------------------------------------------------------------------------------ UPSCALE
NEAREST, BILINEAR, BICUBIC, ALIGN_CORNERS = 0, 1, 2, 1 << 8


def _nearest_index(n_dst, n_src):
    sf = np.float32(n_dst) / np.float32(n_src)
    return (np.arange(n_dst).astype(np.float32) / sf).astype(np.int64)


def upscale_nearest(x, ne):
    """x [N3, N2, H, W] -> shape ne: src index (int64) ((float) i / sf), sf = (float) dst extent / src extent, in every dimension.  A gather: both twins."""
    idx = [_nearest_index(ne[d], x.shape[d]) for d in range(4)]
    assert all(i.max() < n for i, n in zip(idx, x.shape))
    return x[np.ix_(*idx)]


def _lin_axis(n_dst, n_src, f, wrong):
    """(i0, i1, d) of one axis: x = ((float) i + 0.5) / sf - 0.5, x0 = floor(x), x1 = x0 + 1, both clamped to [0, n_src - 1], d = x - (float) clamped x0, clamped to [0, 1]."""
    sf = f(n_dst) / f(n_src)
    i = np.arange(n_dst).astype(f)
    x = i / sf if wrong == "no_half_pixel" else (i + f(0.5)) / sf - f(0.5)
    x0 = np.floor(x).astype(np.int64)
    x1 = x0 + 1
    x0, x1 = np.clip(x0, 0, n_src - 1), np.clip(x1, 0, n_src - 1)
    d = np.clip(x - x0.astype(f), f(0), f(1))
    assert d.dtype == f
    return x0, x1, d


def upscale_bilinear(x, ne, f=np.float32, wrong=None):
    """x [N3, N2, H, W] -> shape ne, no align-corners: bilinear over the last two axes (ggml dims 0 and 1), nearest over the first two.
    value = a (1 - dx) (1 - dy) + b dx (1 - dy) + c (1 - dx) dy + d dx dy, left to right in `f`, a = (x0, y0), b = (x1, y0), c = (x0, y1), d = (x1, y1).
    wrong: "no_half_pixel" samples at x = i / sf (the pixel-centre offset dropped); "nearest" ignores the weights.
    (A twin that takes dx from the UNCLAMPED x0 is no usable wrong twin: x0 leaves [0, W - 1] only as -1, where x0 and x1 clamp to the same pixel, a == b, and
    the weights cancel to within rounding.  The clamped form is still what the contract states and what the kernel does.)"""
    if wrong == "nearest":
        return upscale_nearest(x, ne).astype(f)
    i3, i2 = _nearest_index(ne[0], x.shape[0]), _nearest_index(ne[1], x.shape[1])
    y0, y1, dy = _lin_axis(ne[2], x.shape[2], f, wrong)
    x0, x1, dx = _lin_axis(ne[3], x.shape[3], f, wrong)
    xs = x[np.ix_(i3, i2)].astype(f)
    dy, dx = dy[:, None], dx[None, :]
    a, b = xs[..., y0[:, None], x0[None, :]], xs[..., y0[:, None], x1[None, :]]
    c, d = xs[..., y1[:, None], x0[None, :]], xs[..., y1[:, None], x1[None, :]]
    one = f(1)
    v = a * (one - dx) * (one - dy) + b * dx * (one - dy) + c * (one - dx) * dy + d * dx * dy
    assert v.dtype == f
    return v


def upscale_bilinear_gate(x):
    H, W = x.shape[-2:]
    return (6 * (W + H + 2) + 10) * U * float(np.max(np.abs(x)))
