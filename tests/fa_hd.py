"""FLASH_ATTN_EXT at head sizes 72 / 80 / 88 / 112 (csrc/fattn_hd.hip): what tests/fa_ref.py and tests/fa_d256.py do not know — the head-size FIELD of the form code,
the padded geometry (a K / V row on 16 lanes whatever D / 8 is, so a trip of the split kernel is 64 cells; the matrix cores at 96 / 128 columns), and two more
operand layouts next to the LLM's view into a longer cache:

  cache   K / V [D, n_kv, NKV] with nb[1] = NKV * D * 2, nb[2] = 2 * D: views into a cache 256 cells longer (fa_d256.builder)
  tower   contiguous per head, nb[1] = 2 * D, nb[2] = n_kv * 2 * D (what ggml_cast(permute(k)) gives in clip); Q the permuted view nb[1] = NH * D * 4, nb[2] = D * 4.
          The last head of the last cell ends where the tensor ends.
  gap     head stride 2 * (D + 8) with NaN in the 8 halves between heads, and a NaN guard row behind the last cell — all inside the allocation: a kernel that reads
          a padding lane's bytes reads NaN IN BOUNDS, and 0 x NaN is NaN

Specs, float64 twin, node builder and gates are fa_d256's (Spec takes HD); shared by test_fa_hd_ref_host.py on the CPU and test_gpu_fa_hd.py on the GPU.

Gates: fa_d256's (ORACLE_F16, TWIN_SPLIT, TWIN_MMA, e_gpu <= e_cpu * 1.01 + 1e-12) and fa_ref's INDICATOR_GATE / WITNESS_GATE, unchanged: the padded forms add exact
zeros to the sums of the unpadded size, so the derivations there carry over."""
from dataclasses import dataclass

import numpy as np

import fa_d256 as F2
import fa_ref as FR
import harness as T
import llama_box_amd as L

SIZES = (72, 80, 88, 112)
PADDED = {72: 96, 80: 96, 88: 96, 112: 128}
ROW_LANES = 16   # lanes a K / V row takes in k_fattn_split_hd, D / 8 of them live
TRIP = 64        # cells per workgroup trip of the split kernel: 4 row groups x 4 waves x (64 / ROW_LANES) rows
GAP = 8          # halves between two heads in the gap layout


# ------------------------------------------------------------------------------------------ form codes
def hd_field(D):
    f = FR.fa_constants()["form"]
    return f[f"FA_FORM_HD_{D}"] << f["FA_FORM_HD_SHIFT"]


def hd_mask():
    f = FR.fa_constants()["form"]
    return 7 << f["FA_FORM_HD_SHIFT"]


def form(kernel, mode=0, waves=4, D=80, tail="NONE"):
    """kernels.h: the head-size-64 code of the form with fa_form_hd(D) ORed on."""
    return FR.form(kernel, mode, waves, "F16", 64, tail) | hd_field(D)


def form_name(code):
    f = FR.fa_constants()["form"]
    v = (code & hd_mask()) >> f["FA_FORM_HD_SHIFT"]
    if v == 0:
        return F2.form_name(code)
    D = next(int(k[len("FA_FORM_HD_"):]) for k, x in f.items() if k.startswith("FA_FORM_HD_") and k != "FA_FORM_HD_SHIFT" and x == v)
    return FR.form_name(code & ~hd_mask()).replace("D=64", f"D={D}")


# ------------------------------------------------------------------------------------------ specs
@dataclass(frozen=True)
class Spec(F2.Spec):
    layout: str = "cache"

    @property
    def form(self):
        c = FR.fa_constants()
        tail = "COMBINE" if self.n_splits > 1 else "NONE"
        if self.kernel == "MMA":
            return form("MMA", 1 if self.mask != "none" else 0, c["nw_big"] if self.nq >= c["wg128_min_q"] else c["nw_small"], self.HD, tail)
        return form("SPLIT", 0, 4, self.HD, tail)


@dataclass(frozen=True)
class Case(FR.Case):
    """fa_ref.Case with the padded geometry: fa_ref derives the lanes of a row from D / 8 (9, 10, 11, 14: no divisor of 64); the kernel takes 16."""

    @property
    def trip(self):
        return FR.fa_constants()["bkv"] if self.kernel == "MMA" else FR.fa_constants()["split_ng"] * 4 * (FR.fa_constants()["wave"] // ROW_LANES)


def fr_case(spec):
    c = F2.fr_case(spec)
    return Case(**{k: getattr(c, k) for k in c.__dataclass_fields__})


def _S(D, id, *a, **kw):
    return Spec(f"d{D}_{id}", *a, HD=D, **kw)


# split kernel, every D: one token without a mask on both sides of a trip, and a masked G = 2 decode over three splits
SPLIT_ALL = [_S(D, f"one_token_{n}", "SPLIT", 2, 2, 1, n, mask="none") for D in SIZES for n in (1, 63, 64, 65, 131)] + [
    _S(D, "holes_g2_three_splits", "SPLIT", 4, 2, 1, 333, splits=3) for D in SIZES]
# split kernel, spread over the sizes (each gets three)
SPLIT_ONE = [
    _S(72, "g3", "SPLIT", 6, 2, 1, 67),
    _S(72, "more_splits_than_cells", "SPLIT", 4, 2, 2, 5, splits=8),
    _S(72, "32_tokens", "SPLIT", 4, 2, 32, 260),
    _S(80, "g5", "SPLIT", 5, 1, 1, 67),
    _S(80, "sinks_five_tokens", "SPLIT", 8, 2, 5, 260, splits=2, sinks=True),
    _S(80, "two_batches", "SPLIT", 4, 2, 3, 100, splits=2, nb=2),
    _S(88, "g7", "SPLIT", 7, 1, 1, 67),
    _S(88, "alibi_g8", "SPLIT", 8, 1, 2, 260, alibi=8.0),
    _S(88, "g1_masked", "SPLIT", 2, 2, 1, 131),
    _S(112, "g8", "SPLIT", 8, 1, 1, 67),
    _S(112, "cap50_three_splits", "SPLIT", 16, 8, 1, 333, splits=3, cap=50.0),
    _S(112, "32_tokens", "SPLIT", 4, 2, 32, 260),
]
# matrix cores, every D
MMA_ALL = [_S(D, "mma_33_tile_states", "MMA", 4, 2, 33, 260) for D in SIZES] + [_S(D, "mma_264_nomask", "MMA", 2, 1, 264, 516, mask="none") for D in SIZES]
# matrix cores, one D each; the last two keep the SPLIT form (soft-capping; n_kv % 4 != 0)
MMA_ONE = [
    _S(72, "mma_ragged_cache", "MMA", 4, 2, 64, 68),
    _S(88, "mma_causal_hidden_and_diagonal", "MMA", 4, 2, 64, 260, mask="causal"),
    _S(80, "mma_40_three_splits", "MMA", 4, 2, 40, 1028, splits=3),
    _S(112, "cap_40_tokens_keep_split", "SPLIT", 4, 2, 40, 260, splits=2, cap=50.0),
    _S(72, "kv_262_keeps_split", "SPLIT", 4, 2, 33, 262),
]
# layouts
LAYOUT_SPECS = [_S(D, f"tower_{nq}", "MMA" if nq >= 33 else "SPLIT", 16, 16, nq, 36, mask="none", layout="tower") for D in (72, 88) for nq in (36, 1)] + [
    _S(D, "gap_1", "SPLIT", 4, 2, 1, 131, mask="none", layout="gap") for D in (72, 112)] + [_S(D, "gap_33", "MMA", 4, 2, 33, 260, layout="gap") for D in (72, 112)]
# cell accounting: one split case (two splits, sinks) and one matrix-core case (tile states) per D
CELL_SPECS = [_S(D, "cells_split_sinks_g4", "SPLIT", 8, 2, 5, 260, splits=2, sinks=True) for D in SIZES] + [_S(D, "cells_mma_33", "MMA", 4, 2, 33, 260) for D in SIZES]
RANDOM_SPECS = SPLIT_ALL + SPLIT_ONE + MMA_ALL + MMA_ONE + LAYOUT_SPECS
HIPGRAPH_SPEC = _S(80, "decode_replayed", "SPLIT", 8, 2, 1, 333, splits=3)


# ------------------------------------------------------------------------------------------ layouts
def builder(spec, x, H):
    """-> build(g) for harness.G: the FLASH_ATTN_EXT node of the spec in its layout (x None: shapes and types only, for supports_op)."""
    if spec.layout == "cache":
        return F2.builder(spec, x, H)
    assert spec.tk == L.F16 and spec.tv == L.F16 and not spec.sinks and spec.nb == 1
    D, NH, NKV, nq, nkv = spec.HD, spec.NH, spec.NKV, spec.nq, spec.nkv

    def mask_t(g):
        if spec.mask == "none":
            return None
        return g.new(L.F16, [nkv, (nq + 63) // 64 * 64], x.mask if x else None)

    def tower(g):
        # Q as clip builds it: [D, NH, nq] in memory, permuted to [D, nq, NH]
        tq = H.ggml_permute(g.ctx, g.new(L.F32, [D, NH, nq], np.ascontiguousarray(x.q[0].transpose(1, 0, 2)) if x else None), 0, 2, 1, 3)
        k = g.new(L.F16, [D, nkv, NKV], np.ascontiguousarray(x.Kd.transpose(1, 0, 2)).astype(np.float16) if x else None)
        v = g.new(L.F16, [D, nkv, NKV], np.ascontiguousarray(x.Vd.transpose(1, 0, 2)).astype(np.float16) if x else None)
        tt = tq.contents
        assert list(tt.nb)[:3] == [4, NH * D * 4, D * 4] and list(k.contents.nb)[:3] == [2, 2 * D, nkv * 2 * D]
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, mask_t(g), 1.0 / np.sqrt(D), spec.alibi, spec.cap)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    def gap(g):
        W = NKV * (D + GAP)

        def rows(vals):  # [nkv, NKV, D] float64 -> [nkv + 1, NKV * (D + GAP)] f16: NaN between the heads and in the guard row
            if vals is None:
                return None
            a = np.full((nkv + 1, NKV, D + GAP), np.nan, np.float16)
            a[:nkv, :, :D] = vals.astype(np.float16)
            return a.reshape(nkv + 1, W)

        tq = g.new(L.F32, [D, nq, NH], np.ascontiguousarray(x.q[0]) if x else None)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [W, nkv + 1], rows(x.Kd if x else None)), D, nkv, NKV, 2 * W, 2 * (D + GAP), 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [W, nkv + 1], rows(x.Vd if x else None)), D, nkv, NKV, 2 * W, 2 * (D + GAP), 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, mask_t(g), 1.0 / np.sqrt(D), spec.alibi, spec.cap)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    return tower if spec.layout == "tower" else gap


def run_node(spec, x, target, H, n_threads=4):
    """-> [nb, nq, NH, HD] float32"""
    out = T.run_case(builder(spec, x, H), target, n_threads)[0]
    return np.asarray(out, np.float32).reshape(spec.nb, spec.nq, spec.NH, spec.HD)


_REF = {}


def reference(spec, H):
    """(inputs, oracle result, float64 twin) of a spec, computed once per process and shared by the tests that need them (never written to)."""
    if spec.id not in _REF:
        x = F2.make_inputs(spec)
        ref = run_node(spec, x, "oracle", H)
        exact = F2.twin_of(spec, x)
        ref.setflags(write=False)
        exact.setflags(write=False)
        _REF[spec.id] = (x, ref, exact)
    return _REF[spec.id]


# ------------------------------------------------------------------------------------------ refusals
def refused_builders(H):
    """[(name, build)]: nodes supports_op must keep refusing."""
    out = []
    for hd in (96, 104, 120, 136, 160, 192):
        out.append((f"hd{hd}", F2.builder(F2.Spec(f"hd{hd}", "SPLIT", 4, 2, 1, 64, HD=hd), None, H)))

    def kv_sizes(dk, dv):
        def build(g):
            tq = g.new(L.F32, [dk, 1, 4])
            return H.ggml_flash_attn_ext(g.ctx, tq, g.new(L.F16, [dk, 64, 2]), g.new(L.F16, [dv, 64, 2]), None, 1.0 / np.sqrt(dk), 0.0, 0.0)
        return build

    out += [("k80_v72", kv_sizes(80, 72)), ("k112_v128", kv_sizes(112, 128)), ("k88_v80", kv_sizes(88, 80))]
    for D in SIZES:
        for tk, tv in ((L.BF16, L.BF16), (L.F32, L.F32), (L.F16, L.BF16), (L.F32, L.F16)):
            out.append((f"d{D}_{L.TYPE_NAME[tk]}_{L.TYPE_NAME[tv]}", F2.builder(Spec(f"d{D}_types", "SPLIT", 4, 2, 1, 64, HD=D, tk=tk, tv=tv), None, H)))
        out.append((f"d{D}_g16", F2.builder(Spec(f"d{D}_g16", "SPLIT", 16, 1, 1, 64, HD=D), None, H)))
        out.append((f"d{D}_g9", F2.builder(Spec(f"d{D}_g9", "SPLIT", 9, 1, 1, 64, HD=D), None, H)))
    return out
