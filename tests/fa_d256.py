"""FLASH_ATTN_EXT at head size 256 (Gemma 1 / 2 / 3): what tests/fa_ref.py does not know — the second head-size flag of the form code, soft-capping in the float64
twin — and one node runner that takes a cap, a batch dimension and K / V views into a longer cache (shared by test_fa_d256_ref_host.py on the CPU and
test_gpu_fa_d256.py on the GPU).  Everything else (probe builders, caches, masks, gates of the cell accounting) is imported from fa_ref.

Gates (the project's own, tests/test_gpu_ops.py::test_flash_attn and tests/test_gpu_kv_types.py::test_flash_attn_over_kv_types):
  against the oracle ........ NMSE <= 1e-4 for an f16 cache, <= 1e-3 through the f16 image of another cache type (the oracle asks with an 8-bit query there)
  against the float64 twin .. NMSE <= 1e-9 for the split kernel (f32 throughout), <= 3e-7 for the matrix-core form (P rounded to f16 once: 2^-11 relative per
                              probability, squared and averaged ~ 6e-8), soft-capped or not; and never further from the twin than the oracle: e_gpu <= e_cpu * 1.01 + 1e-12
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

import fa_ref as FR
import harness as T
import llama_box_amd as L

HD = 256
ORACLE_F16, ORACLE_IMAGE = 1e-4, 1e-3
TWIN_SPLIT, TWIN_MMA = 1e-9, 3e-7


# ------------------------------------------------------------------------------------------ form codes
def d256_bit():
    return 1 << FR.fa_constants()["form"]["FA_FORM_D256_BIT"]


def form(kernel, mode=0, waves=4, kv="F16", D=HD, tail="NONE"):
    """kernels.h fa_form_code for any of the three head sizes: fa_ref.form() knows bit 12 (128 / 64); 256 clears it and sets FA_FORM_D256_BIT."""
    if D != 256:
        return FR.form(kernel, mode, waves, kv, D, tail)
    return FR.form(kernel, mode, waves, kv, 64, tail) | d256_bit()


def form_name(code):
    if code & d256_bit():
        return FR.form_name(code & ~d256_bit()).replace("D=64", "D=256")
    return FR.form_name(code)


# ------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Spec:
    id: str
    kernel: str          # the form expected: SPLIT / MMA
    NH: int
    NKV: int
    nq: int
    nkv: int
    splits: int = 0      # option fa_splits (0: the dispatcher's chooser)
    cap: float = 0.0
    alibi: float = 0.0
    sinks: bool = False
    mask: str = "holes"  # none / holes (causal-ish with a masked tail and a hole, as test_flash_attn) / causal (cell c visible to token t when c <= t + 64)
    nb: int = 1          # q.ne[3]
    tk: int = L.F16
    tv: int = L.F16
    HD: int = HD

    @property
    def G(self):
        return self.NH // self.NKV

    @property
    def n_splits(self):
        """What the dispatcher runs with: the option, or fattn_pick_splits' choice (the three branches a head-size-256 node can take)."""
        if self.splits:
            return self.splits
        if self.nq >= FR.fa_constants()["mma_min_q"]:
            return FR.mma_splits(self.nq, self.NH, self.nkv)
        if self.nq > 1:  # "a few tokens, other head sizes"
            return max(1, min(64, min((self.nkv + 255) // 256, max(1, self.nkv // 64))))
        return FR.decode_splits(self.nkv, self.NKV * self.nb, True)

    @property
    def form(self):
        c = FR.fa_constants()
        if self.kernel == "MMA":
            waves = c["nw_big"] if self.nq >= c["wg128_min_q"] else c["nw_small"]
            return form("MMA", 1 if self.mask != "none" else 0, waves, "F16", self.HD, "COMBINE" if self.n_splits > 1 else "NONE")
        return form("SPLIT", 0, 4, "F16", self.HD, "COMBINE" if self.n_splits > 1 else "NONE")

    @property
    def imaged(self):
        return self.tk != L.F16 or self.tv != L.F16


# the trip of k_fattn_split at 256 is 32 cells (a row is 32 lanes, a wave-instruction fetches two rows): a lone cell, both sides of one trip, two trips and a bit
SPLIT_SPECS = [Spec(f"split_one_token_{n}", "SPLIT", 2, 2, 1, n, mask="none") for n in (1, 31, 32, 33, 67)] + [
    Spec("split_gemma2_decode_cap", "SPLIT", 16, 8, 1, 333, splits=3, cap=50.0),
    Spec("split_sinks_g4", "SPLIT", 8, 2, 5, 260, splits=2, sinks=True),
    Spec("split_alibi_g8", "SPLIT", 8, 1, 2, 260, alibi=8.0),
    Spec("split_five_cells_chooser", "SPLIT", 4, 2, 2, 5),
    Spec("split_more_splits_than_cells", "SPLIT", 4, 2, 2, 5, splits=8),  # splits 5 .. 7 are empty: records with max -inf
    Spec("split_two_batches", "SPLIT", 4, 2, 3, 100, splits=2, nb=2),
    Spec("split_g3", "SPLIT", 6, 2, 1, 67),
    Spec("split_g5", "SPLIT", 5, 1, 1, 67),
    Spec("split_g7", "SPLIT", 7, 1, 1, 67),
]
MMA_SPECS = [
    Spec("mma_33_tile_states", "MMA", 4, 2, 33, 260),
    Spec("mma_gemma2_cap_splits", "MMA", 4, 2, 40, 1028, splits=3, cap=50.0),
    Spec("mma_264_nomask", "MMA", 2, 1, 264, 516, mask="none"),
    Spec("mma_ragged_cache", "MMA", 4, 2, 64, 68),
    Spec("mma_causal_hidden_and_diagonal", "MMA", 4, 2, 64, 260, mask="causal"),
    Spec("mma_cap_nomask", "MMA", 2, 1, 33, 132, cap=50.0, mask="none"),  # (the capped score on the path that reads no mask)
]
IMAGE_SPECS = [Spec(f"image_{L.TYPE_NAME[t]}_{nq}", "SPLIT" if nq == 1 else "MMA", 4, 2, nq, 260, tk=t, tv=t) for t in (L.Q8_0, L.Q4_0) for nq in (1, 33)]


# ------------------------------------------------------------------------------------------ inputs
@dataclass
class Inputs:
    q: np.ndarray        # [nb, NH, nq, HD] f32
    kraw: np.ndarray     # cache rows [NCTX, ...] in the cache type
    vraw: np.ndarray
    Kd: np.ndarray       # [nkv, NKV, HD] float64: the values the kernel form sees
    Vd: np.ndarray
    mask: object         # [MR, nkv] f16 or None
    sinks: object
    NCTX: int


def mask_of(spec):
    if spec.mask == "none":
        return None
    nq, nkv = spec.nq, spec.nkv
    m = np.full(((nq + 63) // 64 * 64, nkv), -np.inf, np.float16)
    for t in range(nq):
        if spec.mask == "causal":
            m[t, : min(nkv, t + 65)] = 0
        else:
            m[t, : max(1, nkv - nq + t + 1 - min(17, nkv // 4))] = 0  # (a masked tail of padding cells; a five-cell cache keeps three or four visible)
            if nkv > 8:
                m[t, 5] = -np.inf
    return m


def _cache(t, x, n_extra, width):
    """x [nkv, width] f32 -> (rows [nkv + n_extra, bytes] of the cache tensor, the values an f16 kernel sees of them, float64)."""
    pad = np.zeros((n_extra, width), np.float32)
    full = np.concatenate([x, pad])
    if t == L.F16:
        raw = full.astype(np.float16)
        return raw, raw[: len(x)].astype(np.float64)
    lib = T.oracle()
    src = np.ascontiguousarray(full, np.float32)
    raw = np.zeros(FR.row_bytes(t, src.size), np.uint8)
    lib.oracle_quantize_row(t, src.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p), src.size)
    back = np.zeros(src.size, np.float32)
    lib.oracle_dequantize_row(t, raw.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p), src.size)
    back = back.astype(np.float16).astype(np.float64).reshape(full.shape)  # the f16 image: level * d rounded once
    return raw.reshape(len(full), -1), back[: len(x)]


def make_inputs(spec):
    """Random data; K / V are views of a cache 256 cells longer than nkv (as test_flash_attn)."""
    rng = np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(spec.id)))
    W = spec.NKV * spec.HD
    q = rng.standard_normal((spec.nb, spec.NH, spec.nq, spec.HD)).astype(np.float32)
    kx = rng.standard_normal((spec.nkv, W)).astype(np.float16).astype(np.float32)
    vx = rng.standard_normal((spec.nkv, W)).astype(np.float16).astype(np.float32)
    kraw, Kd = _cache(spec.tk, kx, 256, W)
    vraw, Vd = _cache(spec.tv, vx, 256, W)
    sinks = rng.standard_normal(spec.NH).astype(np.float32) if spec.sinks else None
    return Inputs(q, kraw, vraw, Kd.reshape(spec.nkv, spec.NKV, spec.HD), Vd.reshape(spec.nkv, spec.NKV, spec.HD), mask_of(spec), sinks, spec.nkv + 256)


# ------------------------------------------------------------------------------------------ the float64 twin with soft-capping
def twin(q, Kd, Vd, mask, scale, cap=0.0, sinks=None, alibi=0.0):
    """fa_ref.twin plus the op's soft-capping: s = cap * tanh(s * scale / cap) before the mask.  q [NH, nq, HD] -> out [nq, NH, HD] float64."""
    if cap == 0.0:
        return FR.twin(q, Kd, Vd, mask, scale, sinks, alibi)[0]
    NH, nq, D = q.shape
    nkv, NKV, _ = Kd.shape
    G = NH // NKV
    q16 = q.astype(np.float16).astype(np.float64)
    mk = mask[:nq].astype(np.float64) if mask is not None else np.zeros((nq, nkv))
    out = np.zeros((nq, NH, D))
    n2 = 1 << int(np.floor(np.log2(NH)))
    for h in range(NH):
        slope = 1.0
        if alibi > 0:
            slope = (2.0 ** (-alibi / n2)) ** (h + 1) if h < n2 else (2.0 ** (-alibi / 2 / n2)) ** (2 * (h - n2) + 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = cap * np.tanh(q16[h] @ Kd[:, h // G].T * scale / cap) + slope * mk
            m = s.max(axis=1)
            if sinks is not None:
                m = np.maximum(m, float(sinks[h]))
            p = np.exp(s - m[:, None])
            d = p.sum(axis=1) + (np.exp(float(sinks[h]) - m) if sinks is not None else 0.0)
            out[:, h] = (p @ Vd[:, h // G]) / d[:, None]
    return out


def twin_of(spec, x):
    """-> [nb, nq, NH, HD] float64"""
    return np.stack([twin(x.q[b], x.Kd, x.Vd, x.mask, 1.0 / np.sqrt(spec.HD), spec.cap, x.sinks, spec.alibi) for b in range(spec.nb)])


# ------------------------------------------------------------------------------------------ the node
def builder(spec, x, H):
    """-> build(g) for harness.G: the FLASH_ATTN_EXT node of the spec (x None: shapes and types only, for supports_op)."""
    D, NH, NKV, nq, nkv = spec.HD, spec.NH, spec.NKV, spec.nq, spec.nkv
    NCTX = nkv + 256

    def build(g):
        tq = g.new(L.F32, [D, nq, NH, spec.nb], np.ascontiguousarray(x.q) if x else None)
        kc = g.new(spec.tk, [NKV * D, NCTX], x.kraw if x else None)
        vc = g.new(spec.tv, [NKV * D, NCTX], x.vraw if x else None)
        k = H.ggml_view_3d(g.ctx, kc, D, nkv, NKV, FR.row_bytes(spec.tk, NKV * D), FR.row_bytes(spec.tk, D), 0)
        v = H.ggml_view_3d(g.ctx, vc, D, nkv, NKV, FR.row_bytes(spec.tv, NKV * D), FR.row_bytes(spec.tv, D), 0)
        m = None
        if spec.mask != "none":
            MR = (nq + 63) // 64 * 64
            m = g.new(L.F16, [nkv, MR], x.mask if x else None)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, m, 1.0 / np.sqrt(D), spec.alibi, spec.cap)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        if spec.sinks:
            H.ggml_flash_attn_ext_add_sinks(r, g.new(L.F32, [NH], x.sinks if x else None))
        return r

    return build


def supported(backend, H, build):
    """ggml_backend_dev_supports_op of the node `build` makes — nothing is allocated, uploaded or launched."""
    g = T.G(backend)
    try:
        return bool(H.ggml_backend_dev_supports_op(backend.dev, build(g)))
    finally:
        g.free()


def run_node(spec, x, target, H, n_threads=4):
    """-> [nb, nq, NH, HD] float32"""
    out = T.run_case(builder(spec, x, H), target, n_threads)[0]
    return np.asarray(out, np.float32).reshape(spec.nb, spec.nq, spec.NH, spec.HD)


def fr_case(spec):
    """The fa_ref.Case of a spec, for its probe builders (their form property does not know head size 256: use Spec.form)."""
    return FR.Case(spec.id, spec.kernel, 1 if spec.kernel == "MMA" and spec.mask != "none" else 0, 4 if spec.kernel == "SPLIT" else 2, "COMBINE" if spec.n_splits > 1 else "NONE", spec.HD, spec.NH,
                   spec.NKV, spec.nq, spec.nkv, kv=L.F16, splits=spec.splits, masked=spec.mask != "none", sinks=spec.sinks, alibi=spec.alibi)
