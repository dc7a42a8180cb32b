"""NumPy twins of csrc/ops_act.hip: NORM, GELU / GELU_QUICK / GELU_ERF and the gated units REGLU / GEGLU / GEGLU_QUICK / GEGLU_ERF, written from the
arithmetic DESIGN.md §4h states (ggml-cpu's, restated from memory).  The CPU oracle has none of these ops, so these twins are the reference;
tests/test_act_norm_ref_host.py checks them on the CPU, tests/test_gpu_act_norm.py judges the kernels.

GELU and GELU_QUICK are TABLES in ggml-cpu: 65 536 f16 results indexed by the f16 rounding of the argument, filled at start-up with the process's own
tanhf / expf.  The backend's host code fills the same tables with the same calls; so does tables() here, through ctypes, from the same libm.so.6 in this
process, in the same f32 operation order.  Kernel and twin therefore agree bit for bit or one of them is wrong — no tolerance is involved.

Arrays are in NumPy order (the reverse of ggml's ne[]), as in ops_ref.py.
"""
import ctypes
import functools
import math
import os
import re

import numpy as np

import llama_box_amd as L
from ops_ref import Case, _as_view, bits, catalogue, f32, f32_ulp, row_distance, seeded, ulp_distance  # noqa: F401  (re-exported for the two test files)

OP_NORM, OP_UNARY, OP_GLU = 23, 78, 87  # enum ggml_op (include/ggml_abi.h); test_act_norm_ref_host.py checks them against ggml_op_name
UNARY = {"GELU": 8, "GELU_QUICK": 9, "GELU_ERF": 14}
GLU = {"REGLU": 0, "GEGLU": 1, "SWIGLU": 2, "SWIGLU_OAI": 3, "GEGLU_ERF": 4, "GEGLU_QUICK": 5}
GLU_BUILDER = {"REGLU": "reglu", "GEGLU": "geglu", "GEGLU_ERF": "geglu_erf", "GEGLU_QUICK": "geglu_quick"}
SQRT_2_OVER_PI, GELU_COEF_A, GELU_QUICK_COEF, SQRT_1_2 = f32(0.79788456080286535588), f32(0.044715), f32(-1.702), f32(0.70710678118654752440)


# ------------------------------------------------------------------------------------------------ the two tables
@functools.lru_cache(maxsize=None)
def _libm():
    m = ctypes.CDLL("libm.so.6")
    for fn in (m.tanhf, m.expf):
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float]
    return m


def _map_f32(fn, x):
    return np.array([fn(float(v)) for v in x], np.float32)


def all_f16():
    """f32(f16 pattern i) for i = 0 .. 65535."""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tables():
    """(T_gelu, T_quick) as uint16[65536], each expression left to right in f32 (every NumPy operation below is one IEEE f32 operation):
    T_gelu[i]  = f16(0.5f * h * (1.0f + tanhf(0.79788456f * h * (1.0f + 0.044715f * h * h))))
    T_quick[i] = f16(h * (1.0f / (1.0f + expf(-1.702f * h))))            with h = f32(f16 pattern i)"""
    h = all_f16()
    one, half = f32(1.0), f32(0.5)
    with np.errstate(all="ignore"):
        inner = SQRT_2_OVER_PI * h * (one + GELU_COEF_A * h * h)
        g = half * h * (one + _map_f32(_libm().tanhf, inner))
        q = h * (one / (one + _map_f32(_libm().expf, GELU_QUICK_COEF * h)))
        assert inner.dtype == g.dtype == q.dtype == np.float32
        return g.astype(np.float16).view(np.uint16), q.astype(np.float16).view(np.uint16)


@functools.lru_cache(maxsize=None)
def functions_f64():
    """The two functions at every f16 argument, evaluated in float64."""
    with np.errstate(all="ignore"):
        h = all_f16().astype(np.float64)
        g = 0.5 * h * (1.0 + np.tanh(float(SQRT_2_OVER_PI) * h * (1.0 + float(GELU_COEF_A) * h * h)))
        q = h * (1.0 / (1.0 + np.exp(float(GELU_QUICK_COEF) * h)))
    return g, q


def tables_f64():
    """... rounded once to f16: what the tables would be without f32 intermediates."""
    with np.errstate(all="ignore"):
        return tuple(v.astype(np.float16).view(np.uint16) for v in functions_f64())


def _f16_index(x32):
    with np.errstate(all="ignore"):
        return np.asarray(x32, np.float32).astype(np.float16).view(np.uint16)  # IEEE round to nearest even, inf from 65520 on


# ------------------------------------------------------------------------------------------------ twins
def gelu(x):
    """x <= -10 -> +0, x >= 10 -> x, else the table at the f16 rounding of x; a NaN fails both comparisons and takes the table."""
    x = np.asarray(x, np.float32)
    t = tables()[0][_f16_index(x)].view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.where(x <= f32(-10.0), f32(0.0), np.where(x >= f32(10.0), x, t)).astype(np.float32)


def gelu_quick(x):
    """The table and nothing else: |x| >= 65520 reads the entry of +-inf (inf and NaN), as the reference does."""
    return tables()[1][_f16_index(x)].view(np.float16).astype(np.float32)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu_erf64(x):
    """0.5 x (1 + erf(x / sqrt 2)) in float64 — with the f32 constant the definition multiplies by."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return 0.5 * x * (1.0 + _erf(x * float(SQRT_1_2)))


def relu(x):
    x = np.asarray(x, np.float32)
    return np.where(x > 0, x, f32(0.0)).astype(np.float32)


def glu(op, x, g):
    """act(x) * g.  REGLU / GEGLU / GEGLU_QUICK: one f32 product after an exact value (f32, compared by bits); GEGLU_ERF: float64."""
    g32 = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        if op == "GEGLU_ERF":
            return gelu_erf64(x) * g32.astype(np.float64)
        act = {"REGLU": relu, "GEGLU": gelu, "GEGLU_QUICK": gelu_quick}[op](x)
        return (act * g32).astype(np.float32)


def norm(x, eps, w=None, b=None):
    """ggml_compute_forward_norm_f32's order: mean = f32(sum of (double) x / n); v = x - mean in f32; var = sum of (double) f32(v * v) / n;
    y = v / sqrt(var + eps) [* w] [+ b].  The f32 steps the definition fixes before the statistics (mean, v, the squares) are f32 here; the variance and
    everything after it is float64.  A constant row is v = 0: y = 0, or 0 * inf = NaN when eps is 0."""
    x32 = np.asarray(x, np.float32)
    n = x32.shape[-1]
    with np.errstate(all="ignore"):
        mean = (x32.astype(np.float64).sum(axis=-1, keepdims=True) / n).astype(np.float32)
        v = (x32 - mean).astype(np.float32)
        sq = (v * v).astype(np.float32).astype(np.float64)
        var = sq.sum(axis=-1, keepdims=True) / n
        y = v.astype(np.float64) * (1.0 / np.sqrt(var + float(f32(eps))))
        if w is not None:
            y = y * np.asarray(w, np.float32).astype(np.float64)
        if b is not None:
            y = y + np.asarray(b, np.float32).astype(np.float64)
    return y


def layer_norm64(x, eps):
    """The textbook LayerNorm, float64 throughout."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        c = x - x.mean(axis=-1, keepdims=True)
        return c / np.sqrt((c * c).mean(axis=-1, keepdims=True) + eps)


# ------------------------------------------------------------------------------------------------ gates
U23, U24 = 2.0 ** -23, 2.0 ** -24
# NORM, as a fraction of the row's largest |y| (row_distance) from norm() above.  What the kernel does that norm() does not:
#   * its double partial sums run in another order, which can move the f32 MEAN onto its neighbour: v = x - mean moves by one ulp of the mean,
#     2^-23 |mean|, for every element — 2^-23 |mean| / max |x - mean| of the row's largest result.  That is the per-case term (Case.extra, norm_extra());
#     it is the definition's own conditioning (a row whose mean is 1000 times its spread has lost 10 bits before any kernel touches it);
#   * it rounds the variance to f32, where the order of ITS partial sums decides between two neighbours when the sum sits on a rounding boundary: either is
#     within 2^-24 of var, and the root halves that in the scale: 0.5 units of 2^-24;
#   * var + eps (0.5 after the root), sqrtf (1), the reciprocal (1) and v * scale (1) are four more f32 roundings.
#   Together 4 units of 2^-24 = 2 * 2^-23 of every result, hence of the row's largest.  ops_ref.ALLOWANCE["rms_norm"] reasons the same way about the f32 mean of
#   squares; there the roundings both sides perform sit in the oracle's baseline, here no oracle computes NORM and they are counted.
NORM_GATE = 2 * U23
# GELU_ERF / GEGLU_ERF: r = (0.5 x) (1 + erff(x c)) [g].  The result cancels for negative x (1 + erf -> 0), so ulps of r say nothing: the gate is on the ABSOLUTE
# error, |err| <= ERF_K 2^-24 |x| |g| + 1 ulp(r).  erff is the one library call; no accuracy table of the device library ships with the toolchain, the bound taken
# is the one it is written to, OpenCL's full profile: erf <= 16 ulp (ops_ref.ALLOWANCE takes tanh's 5 ulp from the same place).  |erf| <= 1, so the call is off
# by <= 16 * 2^-24, times 0.5 |x| |g|: 8 units.  The rounded argument x c moves erf by <= 1.13 exp(-t^2) t 2^-24 < 0.5 * 2^-24: a quarter unit.  1 + erff is one
# rounding of a value <= 2: half a unit after the 0.5.  That is under 9 of the 16 units; the two products (by 0.5 x, by g) are roundings of the result: 1 ulp(r).
ERF_K = 16.0


def norm_extra(x):
    """2^-23 |mean| / max |x - mean|, the largest over the rows of x, with the f32 mean and differences of the definition (0 for a row without spread: its
    results are 0 or NaN whatever the mean's last bit)."""
    x32 = np.asarray(x, np.float32).reshape(-1, np.shape(x)[-1])
    with np.errstate(all="ignore"):
        mean = (x32.astype(np.float64).sum(axis=-1, keepdims=True) / x32.shape[-1]).astype(np.float32)
        spread = np.max(np.abs((x32 - mean).astype(np.float32).astype(np.float64)), axis=-1)
        r = np.where(spread > 0, np.abs(mean[:, 0].astype(np.float64)) / np.where(spread > 0, spread, 1.0), 0.0)
    return float(U23 * np.max(r))


def erf_excess(got, x, g=None):
    """|got - twin| / (ERF_K 2^-24 |x| |g| + ulp(twin)), element by element: <= 1 passes.  NaN on both sides and equal values count 0."""
    x32 = np.asarray(x, np.float32)
    g64 = np.ones(x32.shape) if g is None else np.asarray(g, np.float32).astype(np.float64)
    got = np.asarray(got, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        ref = gelu_erf64(x32) * g64
        tol = ERF_K * U24 * np.abs(x32.astype(np.float64)) * np.abs(g64) + f32_ulp(ref)
        same = (np.isnan(got) & np.isnan(ref)) | (got == ref) | (got == ref.astype(np.float32).astype(np.float64))
        d = np.where(same, 0.0, np.abs(got - ref) / tol)
    return np.where(np.isnan(d), np.inf, d)


# ------------------------------------------------------------------------------------------------ the constants the shapes come from
def act_limits():
    """The launcher constants of csrc/ops_act.hip the edge shapes below follow, parsed as ops_ref.ops_limits() parses ops.hip: a retuned launcher then names
    the stale shape.  If an expression is rewritten, the pattern that names it here is the line to edit.
      grid_cap     most workgroups of launch_gelu before the grid-stride loop takes a second stride      `(n + 255) / 256, 2048)`
      norm_trip    f32 values one trip of k_norm's float4 loops covers = the widest row kept in registers  `i0 += 1024` (float4s), `n4 <= 1024`
      glu_chunk    values of one grid.y chunk of k_glu                                                   `(nc + 1023) / 1024`"""
    with open(os.path.join(L.REPO, "llama_box_amd", "csrc", "ops_act.hip")) as f:
        src = f.read()

    def body(name):
        m = re.search(r"\n(?:void|bool) " + name + r"\(.*?\n}\n", src, re.S)
        assert m, f"{name} not found in ops_act.hip — edit tests/act_norm_ref.py: act_limits"
        return m.group(0)

    def kernel(name):
        m = re.search(r"__global__ void [^\n]*\b" + name + r"\(.*?\n}\n", src, re.S)
        assert m, f"{name} not found in ops_act.hip — edit tests/act_norm_ref.py: act_limits"
        return m.group(0)

    def one(text, pattern, what):
        m = re.findall(pattern, text)
        assert len(set(m)) == 1, f"{what}: pattern {pattern!r} matches {m} — the expression moved, edit tests/act_norm_ref.py: act_limits"
        return m[0]

    cap = int(one(body("launch_gelu"), r"\(n \+ 255\) / 256, (\d+)\)", "grid cap of launch_gelu"))
    trip = int(one(kernel("k_norm"), r"i0 < n4; i0 \+= (\d+)\)", "float4 trip of k_norm"))
    reg = int(one(kernel("k_norm"), r"if \(n4 <= (\d+)\)", "k_norm: rows kept in registers"))
    assert reg == trip, "k_norm: the register path holds exactly one trip"
    up, chunk = one(body("launch_glu"), r"\(nc \+ (\d+)\) / (\d+)\)", "k_glu chunk")
    assert int(up) + 1 == int(chunk)
    per_thread = int(one(kernel("k_glu"), r"blockIdx\.y \* 256 \+ threadIdx\.x\) \* (\d+);", "k_glu values per thread"))
    assert 256 * per_thread == int(chunk), "k_glu: a chunk is 256 threads x the values of one thread"
    return {"grid_cap": cap, "norm_trip": trip * 4, "glu_chunk": int(chunk)}


# the shapes the tests use; test_act_norm_ref_host.py checks them against act_limits()
GELU_N = 2048 * 256 + 257   # a second, partial stride of the grid-stride loop
NORM_NE0 = (1, 3, 100, 4096, 4100, 8192)
GLU_NC = (6, 1024, 1028, 2050)


def shapes_from(lim):
    return {"GELU_N": lim["grid_cap"] * 256 + 257,
            "NORM_NE0": (1, 3, 100, lim["norm_trip"], lim["norm_trip"] + 4, 2 * lim["norm_trip"]),
            "GLU_NC": (6, lim["glu_chunk"], lim["glu_chunk"] + 4, 2 * lim["glu_chunk"] + 2)}


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def gelu_input():
    """One tensor of GELU_N values: every f16 pattern widened; for 4096 adjacent f16 pairs spread over the exponents the f32 midpoint (a tie) and its two
    f32 neighbours; both sides of +-10; the f16 overflow boundary; ops_ref.catalogue(); seeded fill."""
    up, dn = f32(np.inf), f32(-np.inf)
    h_all = all_f16()
    lo = np.linspace(1, 0x7BFE, 4096).astype(np.uint16)  # positive finite patterns from the smallest subnormal to the one below 65504; the pair is (lo, lo + 1)
    sign = (np.arange(4096) & 1).astype(np.uint16) << 15
    a = (lo | sign).view(np.float16).astype(np.float32)
    b = ((lo + 1).astype(np.uint16) | sign).view(np.float16).astype(np.float32)
    mid = ((a.astype(np.float64) + b.astype(np.float64)) / 2).astype(np.float32)  # exact: 12 significant bits
    ties = np.concatenate([mid, np.nextafter(mid, up), np.nextafter(mid, dn)])
    ten = np.array([10.0, -10.0, np.nextafter(f32(10), up), np.nextafter(f32(10), dn), np.nextafter(f32(-10), up), np.nextafter(f32(-10), dn)], np.float32)
    big = np.array([65504.0, 65519.996, 65520.0, 1e30, -65504.0, -65519.996, -65520.0, -1e30], np.float32)
    head = np.concatenate([h_all, ties, ten, big, catalogue()])
    return np.concatenate([head, seeded(np.random.default_rng(8100), GELU_N - len(head), span=12.0)]).astype(np.float32)


def glu_operands(nc, rows, seed):
    """x takes the catalogue, both sides of +-10 and seeded values of the GELU range; g exact values among Gaussian ones (a subnormal act(x) times a large g
    would turn f32's absolute grid into a relative error of the product, the definition's own)."""
    rng = np.random.default_rng(seed)
    ten = np.array([10.0, -10.0, np.nextafter(f32(10), f32(np.inf)), np.nextafter(f32(10), f32(-np.inf)), np.nextafter(f32(-10), f32(np.inf)), np.nextafter(f32(-10), f32(-np.inf))], np.float32)
    x = np.resize(np.concatenate([catalogue(), ten, seeded(rng, rows * nc, span=12.0)]), (rows, nc)).astype(np.float32)
    g = (rng.standard_normal((rows, nc)) * 2).astype(np.float32)
    exact = np.array([0.0, -0.0, 1.0, -1.0, 0.5, np.inf, -np.inf, np.nan], np.float32)
    g[0, ::5] = np.resize(exact, len(g[0, ::5]))
    return x, g
