"""NumPy twins of csrc/diffusion.hip: GROUP_NORM, TIMESTEP_EMBEDDING, DIAG_MASK_INF and LEAKY_RELU, written from the arithmetic DESIGN.md §4n states (ggml-cpu's,
restated from memory).  Nothing on record pins these ops — the CPU oracle has none of them —, so these twins are the reference, as conv_ref.py is for the tower
ops; tests/test_diffusion_ref_host.py checks them on the CPU, tests/test_gpu_diffusion.py judges the kernels.

Arrays are in NumPy order (the reverse of ggml's ne[]): a [W, H, C, N] tensor is x[N, C, H, W].

GROUP_NORM is NORM with "row" read as "group" (act_norm_ref.norm: the f32 steps the definition fixes — the mean, x - mean, the squares — in f32, the variance and
everything after it in float64), and its gate is NORM's, group by group: act_norm_ref.NORM_GATE + norm_extra(group).  The kernels do the same double sums in
another order, which is all that reasoning rests on, so no new number is introduced.

DIAG_MASK_INF and LEAKY_RELU are f32 twins compared by bits.  LEAKY_RELU is fmaxf(x, 0) + slope * fminf(x, 0) with two roundings; C leaves the sign of fmaxf(-0, +0)
open, the twin (and the kernel, which spells the two selections out) takes IEEE 754-2019's maximumNumber / minimumNumber: -0 ranks below +0 and a NaN gives way to
the number, so x = -0 is (+0) + slope * (-0) and x = NaN is (+0) + slope * (+0).

TIMESTEP_EMBEDDING: half = dim // 2; for j < half: freq = expf(-logf(max_period) * j / half); arg = t * freq; y[j] = cosf(arg); y[j + half] = sinf(arg); a row is dim
rounded up to even wide and every column from 2 * half on is 0.  The twin is float64 from the definition's f32 inputs (t, and max_period, j, half as exact
integers).  The results cancel near their zeros, so the gate is on the ABSOLUTE error, |err| <= TE_ABS + te_rel(max_period) * |arg|, derived as act_norm_ref.ERF_K
is: the device library is written to OpenCL's full-profile bounds (exp / log 3 ulp, sin / cos 4 ulp), the f32 roundings are counted one by one, in units of
2^-23 (one ulp of a value in [1, 2); half of that is the bound of one rounding to nearest):
  * e = -logf(max_period) * j / half: logf is off by <= 3 ulp, the product and the quotient round once each (0.5 + 0.5): e is off by <= 4 * 2^-23 |e|, and
    |e| <= ln(max_period);
  * freq = expf(e): the argument's error moves exp by |e| times its relative error, <= 4 ln(max_period) * 2^-23 of freq; the call itself is off by <= 3 ulp;
  * arg = t * freq rounds once: 0.5.  Together arg is off by <= (4 ln(max_period) + 3.5) * 2^-23 |arg|; te_rel takes 4 ln(max_period) + 4, the half unit
    covering the products of these terms;
  * cos and sin have slope <= 1, so the result moves by no more than arg does; the call is off by <= 4 ulp of a result <= 1: TE_ABS = 4 * 2^-23.
The frequencies are evaluated on the device (DESIGN.md §4n says why), so the |arg| term is the whole of what is not bit-exact before the call: at t = 999, j = 0
and max_period = 10 000 the gate is 999 * 40.8 * 2^-23 = 4.9e-3.
"""
import math
import os
import re

import numpy as np

import act_norm_ref as A
import llama_box_amd as L
from ops_ref import bits, f32, row_distance, tile_to  # noqa: F401  (re-exported for the two test files)

OP_GROUP_NORM, OP_DIAG_MASK_INF, OP_DIAG_MASK_ZERO, OP_TIMESTEP_EMBEDDING, OP_LEAKY_RELU = 26, 43, 44, 64, 66  # enum ggml_op; test_diffusion_ref_host.py checks them against ggml_op_name

# the two constants of csrc/kernels.h the edge shapes follow; test_diffusion_ref_host.py holds them equal to the source's
GN_CHUNK = 4096          # MI_GN_CHUNK: values of one chunk of the split form
GN_RESIDENT_MAX = 40960  # MI_GN_RESIDENT_MAX: values of the largest group the resident form holds

U23 = 2.0 ** -23
TE_ABS = 4 * U23


def te_rel(max_period):
    return (4.0 * math.log(max_period) + 4.0) * U23


def source_constants():
    """{name: value} of the MI_GN_* #defines of csrc/kernels.h."""
    with open(os.path.join(L.REPO, "llama_box_amd", "csrc", "kernels.h")) as f:
        src = f.read()
    out = {k: int(v) for k, v in re.findall(r"^#define (MI_GN_[A-Z_]+) (\d+)$", src, re.M)}
    assert {"MI_GN_CHUNK", "MI_GN_RESIDENT_MAX", "MI_GN_ROUTED_MAX"} <= set(out), out
    return out


# ------------------------------------------------------------------------------------------------ GROUP_NORM
def group_ranges(C, G):
    """[(c0, c1)] of the G groups over C channels: cpg = ceil(C / G), group g is [g cpg, min((g + 1) cpg, C)).  None where a group would be empty
    ((G - 1) cpg >= C: ggml-cpu divides by a non-positive count there; the backend refuses the node) or G <= 0."""
    if G <= 0 or C <= 0:
        return None
    cpg = -(-C // G)
    if (G - 1) * cpg >= C:
        return None
    return [(g * cpg, min((g + 1) * cpg, C)) for g in range(G)]


def _groups(x, G):
    x = np.asarray(x)
    assert x.ndim == 4
    r = group_ranges(x.shape[1], G)
    assert r is not None, (x.shape, G)
    return [(n, c0, c1) for n in range(x.shape[0]) for c0, c1 in r]


def group_norm(x, G, eps):
    """float64 [N, C, H, W]: act_norm_ref.norm over every group's values as one row."""
    x32 = np.asarray(x, np.float32)
    y = np.empty(x32.shape, np.float64)
    for n, c0, c1 in _groups(x32, G):
        y[n, c0:c1] = A.norm(x32[n, c0:c1].reshape(1, -1), eps).reshape(x32[n, c0:c1].shape)
    return y


def group_norm64(x, G, eps):
    """The textbook GroupNorm, float64 throughout (the ceil rule for the channel ranges)."""
    x = np.asarray(x, np.float64)
    y = np.empty(x.shape, np.float64)
    with np.errstate(all="ignore"):
        for n, c0, c1 in _groups(x, G):
            v = x[n, c0:c1]
            c = v - v.mean()
            y[n, c0:c1] = c / np.sqrt((c * c).mean() + eps)
    return y


def group_norm_excess(got, x, G, eps):
    """(worst fraction of the gate, worst distance, its gate) over the groups: a group's distance is max |got - twin| over the group's largest |twin|
    (ops_ref.row_distance with the group as the row), its gate NORM_GATE + norm_extra(group)."""
    x32 = np.asarray(x, np.float32)
    got = np.asarray(got).reshape(x32.shape)
    want = group_norm(x32, G, eps)
    worst = (0.0, 0.0, A.NORM_GATE)
    for n, c0, c1 in _groups(x32, G):
        d = float(row_distance(got[n, c0:c1].reshape(1, -1), want[n, c0:c1].reshape(1, -1))[0])
        gate = A.NORM_GATE + A.norm_extra(x32[n, c0:c1].reshape(1, -1))
        if d / gate >= worst[0]:
            worst = (d / gate, d, gate)
    return worst


def channel_binary(op, a, v):
    """MUL / ADD of a [N, C, H, W] with a per-channel vector ([1, 1, C, 1] in ggml's order): one f32 operation, ops_ref.binary's."""
    a = np.asarray(a, np.float32)
    t = tile_to(np.asarray(v, np.float32).reshape(1, -1, 1, 1), a.shape)
    with np.errstate(all="ignore"):
        return (a * t if op == "mul" else a + t).astype(np.float32)


# ------------------------------------------------------------------------------------------------ DIAG_MASK_INF, LEAKY_RELU
def diag_mask_inf(x, n_past):
    """x[..., j, i] = -inf where i > n_past + j (i: dim 0, the column; j: dim 1, the row), the value elsewhere."""
    x = np.array(x, np.float32)
    j, i = np.indices(x.shape[-2:])
    x[..., i > n_past + j] = -np.inf
    return x


def leaky_relu(x, slope):
    """maximumNumber(x, +0) + slope * minimumNumber(x, +0) in f32, the product and the sum one rounding each."""
    x = np.asarray(x, np.float32)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        hi = np.where(x > 0, x, zero).astype(np.float32)
        lo = np.where(x <= 0, x, zero).astype(np.float32)  # (-0 stays -0, +0 stays +0, a NaN becomes +0)
        q = (f32(slope) * lo).astype(np.float32)
        return (hi + q).astype(np.float32)


# ------------------------------------------------------------------------------------------------ TIMESTEP_EMBEDDING
def timestep_embedding(t, dim, max_period):
    """-> (y float64 [N, dim rounded up to even], |arg| float64 of the same shape: what the gate's second term multiplies; 0 in the zero columns)."""
    t = np.asarray(t, np.float32).astype(np.float64).reshape(-1)
    half = dim // 2
    width = dim + (dim & 1)
    y = np.zeros((len(t), width), np.float64)
    arg_abs = np.zeros((len(t), width), np.float64)
    j = np.arange(half, dtype=np.float64)
    arg = t[:, None] * np.exp(-math.log(max_period) * j / half)[None, :]
    y[:, :half], y[:, half:2 * half] = np.cos(arg), np.sin(arg)
    arg_abs[:, :half] = arg_abs[:, half:2 * half] = np.abs(arg)
    return y, arg_abs


def timestep_excess(got, t, dim, max_period):
    """|got - twin| / (TE_ABS + te_rel(max_period) |arg|), element by element: <= 1 passes; a zero column must be exactly +0 or -0."""
    want, arg_abs = timestep_embedding(t, dim, max_period)
    got = np.asarray(got, np.float32).astype(np.float64).reshape(want.shape)
    d = np.abs(got - want) / (TE_ABS + te_rel(max_period) * arg_abs)
    d[:, 2 * (dim // 2):] = np.where(got[:, 2 * (dim // 2):] == 0, 0.0, np.inf)
    return np.where(np.isnan(d), np.inf, d)
