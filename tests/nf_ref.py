"""Cell accounting for the non-flash attention chain MUL_MAT(K view, q) -> SOFT_MAX(mask, scale) -> MUL_MAT(V^T view, p) -> CONT(PERMUTE), which graph.cpp replaces by
k_attn_nf_list<G> (csrc/attn_nf.hip, 2 .. 32 tokens: one launch over each token's list of visible cells) or k_attn_nf_mma (csrc/fattn_mma.hip, 33 tokens and more: two
matrix-core passes over per-tile visibility states plus the split combine).  Shared by test_nf_ref_host.py (CPU) and test_gpu_nf_cells.py (GPU); modelled on fa_ref.py,
whose probe kinds and gates it takes over:

  indicator  q = 0, V one-hot by residue (pattern A: cell % 128, pattern B: (cell // 128) % 128): every weight is the same p = f16(1 / cnt), so out * denominator counts the
             visible cells per residue.  Gate |out - twin| * den <= 0.01 (fa_ref.INDICATOR_GATE).  The sums are exact in f32 in any order (k * p has at most 11 + 12
             bits), and the twin rounds p to f16 as the CPU's second MUL_MAT rounds its src1 — without that the figure could reach cnt / 2 * 2^-11.  A missing, doubled or
             misplaced cell moves a residue by about 1 while no residue holds more than half of a token's cells (asserted on the inputs).
  witness    q = gamma * K[witness], gamma doubled until the witness leads every other visible score by 60 nats: its probability is exactly 1.0 in f16, every other one
             rounds to 0, the result is the witness' V row.  Gate 1e-6 * max |V| (fa_ref.WITNESS_GATE).  (Blind to a DOUBLED witness: 2 / 2 is 1.0 too — the pair and the
             indicator see that.)
  pair       two cells with the same K row on the two sides of a boundary (group of eight, 256-thread stride, 512, NF_CAP, the 16-cell trip of the scratch path; a 64-cell
             tile end, a split end): 0.5 each, V on a grid of 1 / 64, so (V[a] + V[b]) / 2 is exact.  Same gate.
  random     random data, finite mask values -1.5 and 0.75 in some 64-cell blocks and -0.0 in one; NMSE <= 1e-9 against the CPU oracle (test_non_flash_attention_chain's gate).
No gate here is taken from a kernel's output."""
import dataclasses
import re
from dataclasses import dataclass

import numpy as np

import fa_ref as FR
import llama_box_amd as L
from fa_ref import INDICATOR_GATE, MARGIN_NATS, WITNESS_GATE, Probe, mask_of, mma_splits  # noqa: F401  (re-exported: the gates are fa_ref's)

RANDOM_GATE = 1e-9       # NMSE against the oracle: test_non_flash_attention_chain's
RANDOM_GATE_WO = 5e-6    # ... read through the Q8_K activation of a quantised mat-mul: test_non_flash_attention_chain_into_wo's
HD = 128                 # both forms serve nothing else


# ------------------------------------------------------------------------------------------ constants parsed from the sources
_CONST = None


def nf_constants():
    """What decides which path a token's list takes, read from the expressions in attn_nf.hip / fattn_mma.hip / graph.cpp (the pattern that stops matching names the line
    to edit; EDGE_TABLE in test_nf_ref_host.py says what the cases were laid out for)."""
    global _CONST
    if _CONST is not None:
        return _CONST
    nf, mma, gr = FR._src("attn_nf.hip"), FR._src("fattn_mma.hip"), FR._src("graph.cpp")
    one = lambda text, pat, what: FR._one(text, pat, what + " (tests/nf_ref.py: nf_constants)")
    c = {}
    c["cap"] = int(one(nf, r"#define NF_CAP (\d+) ", "NF_CAP"))
    c["threads"] = int(one(nf, r"__launch_bounds__\((\d+)\) k_attn_nf_list", "workgroup of k_attn_nf_list"))
    strides = set(re.findall(r"for \(int c = tid; c < cnt; c \+= (\d+)\)", nf))
    assert strides == {str(c["threads"])}, f"thread stride over a list: {strides}"
    c["group_max"] = int(one(nf, r"if \(dq_n == 1 && cnt <= (\d+) && nf_groups\)", "cell limit of the group form"))
    c["group"] = int(one(nf, r"const int ngr = \(cnt \+ 7\) / (\d+), gi_l = lane;", "group size"))
    m = one(nf, r"while \(dq < (\d+) && T \* NKV \* dq < (\d+)\) dq \*= 2;", "slices of the head dimensions")
    c["dq_max"], c["dq_wgs"] = int(m[0]), int(m[1])
    c["scratch_trip"] = int(one(nf, r"for \(int c0 = wave \* 4; c0 < cnt; c0 \+= (\d+)\)", "trip of the scratch path"))
    m = one(nf, r"if \(T < (\d+) \|\| T > (\d+) \|\| NKV <= 0", "tokens served by the list form")
    c["t_min"], c["t_max"] = int(m[0]), int(m[1])
    c["g_max"] = int(one(nf, r"if \(G < 1 \|\| G > (\d+)\) return 0;", "query heads per KV head"))
    one(nf, r"if \((n_kv > \(int64_t\) NF_CAP \* T)\) return 0;", "average-row rule")
    m = one(nf, r"if \(G <= (\d+) && rows_per >= (\d+)\) vtp\(std::integral_constant<int, (\d+)>\{\}\);\n\s*else if \(rows_per >= (\d+)\) vtp\(std::integral_constant<int, (\d+)>\{\}\);\n"
                r"\s*else vtp\(std::integral_constant<int, (\d+)>\{\}\);", "rows per wave and block of V^T.p")
    c["rb"] = tuple(int(x) for x in m)
    c["named_row_max"] = int(one(gr, r"lookup_mask_stats\(mask_upload_ptr\(M\), &ms\) && ms\.max_visible > (\d+)\) return false;", "longest row of a named mask"))
    one(gr, r"if \(\(M->type != GGML_TYPE_F16 && M->type != GGML_TYPE_F32\) \|\| (\(K->ne\[1\] % 4\) != 0)", "list scan: four cells per thread")
    # the matrix-core form: tiles and the split chooser (fa_ref parses the same file for FLASH_ATTN_EXT; this is the expression itself, compared with fa_ref.mma_splits on the CPU)
    fc = FR.fa_constants()
    c["bkv"], c["scan_q"], c["mma_min_q"] = fc["bkv"], fc["scan_q"], fc["mma_min_q"]
    m = one(mma, r"const int64_t qt = q\.ne\[1\] >= (\d+) \? (\d+) : (\d+);", "fattn_mma_pick_splits, query tile")
    c["pick_qt"] = tuple(int(x) for x in m)
    c["pick_want"] = int(one(mma, r"int64_t want = \((\d+) \+ wgs - 1\) / wgs;", "fattn_mma_pick_splits, workgroups"))
    m = one(mma, r"want = std::max<int64_t>\(1, std::min<int64_t>\(want, std::min<int64_t>\((\d+), tiles / (\d+)\)\)\);", "fattn_mma_pick_splits, tiles")
    c["pick_max"], c["pick_tiles_per"] = int(m[0]), int(m[1])
    one(mma, r"vt\.ne\[1\] != D \|\| (\(k\.ne\[1\] % 8\) != 0)\) return false;", "attn_nf_mma_applies: eight cells per 16-byte load of V^T")
    m = one(FR._src("fattn.hip"), r"n_splits >= (\d+) && n_splits <= (\d+) && n_rows >= (\d+) && n_rows <", "fattn_combine_rows_applies")
    c["rows"] = tuple(int(x) for x in m)
    _CONST = c
    return c


def dq_of(T, NKV):
    c = nf_constants()
    dq = 1
    while dq < c["dq_max"] and T * NKV * dq < c["dq_wgs"]:
        dq *= 2
    return dq


def rb_of(G, dq):
    g_max, rows_a, rb_a, rows_b, rb_b, rb_c = nf_constants()["rb"]
    rows_per = HD // dq
    return rb_a if G <= g_max and rows_per >= rows_a else (rb_b if rows_per >= rows_b else rb_c)


def path_of(cnt, dq):
    """The device-side branch a token with cnt visible cells takes in k_attn_nf_list."""
    c = nf_constants()
    if cnt == 0:
        return "nan"
    if cnt > c["cap"]:
        return "scratch"
    return "group" if dq == 1 and cnt <= c["group_max"] else "vtp"


def pick_splits(T, NH, nkv):
    """fattn_mma_pick_splits as parsed above."""
    c = nf_constants()
    qt = c["pick_qt"][1] if T >= c["pick_qt"][0] else c["pick_qt"][2]
    wgs = -(-T // qt) * NH
    tiles = -(-nkv // c["bkv"])
    return max(1, min(-(-c["pick_want"] // wgs), c["pick_max"], tiles // c["pick_tiles_per"]))


def rows_combine_applies(T, NH, S):
    lo, hi, rows = nf_constants()["rows"]
    return lo <= S <= hi and T * NH >= rows


# ------------------------------------------------------------------------------------------ the cases
LADDER = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1500, 2100)
LAYOUTS = ("np", "run_aligned", "run_odd", "run_shift", "stride", "partial", "groups64", "run_to_end", "run_from_zero")
MMA_FAMILIES = ("full", "causal_end", "blockdiag", "interleaved", "tile_states")


@dataclass(frozen=True)
class Case:
    id: str
    form: str            # LIST / MMA / DENSE (a shape both forms refuse: the dense kernels)
    NH: int
    NKV: int
    T: int
    nkv: int
    families: tuple      # visibility families of the indicator probe; the first also carries the witness, pair and random probes
    mtype: int = L.F32   # llama.cpp's mask is f32 when flash attention is off; the list form serves f16 too
    dest: str = "copy"   # copy: the CONT copy is the only reader; kqv: kqv is a graph output too; wo: a one-hot Q4_K read-out matrix follows
    scale: float = 0.0   # 0: 1 / sqrt(HD)
    HD: int = 128
    mask_name: str = ""  # (a mask called KQ_mask has upload statistics: a row above 1024 cells keeps the batch on the dense kernels)

    @property
    def G(self):
        return self.NH // self.NKV

    @property
    def dq(self):
        return dq_of(self.T, self.NKV)

    @property
    def sc(self):
        return self.scale or 1.0 / np.sqrt(self.HD)

    @property
    def n_splits(self):
        return mma_splits(self.T, self.NH, self.nkv) if self.form == "MMA" else 1

    @property
    def per(self):
        """MMA: cells per split."""
        B = nf_constants()["bkv"]
        return -(-(-(-self.nkv // B)) // self.n_splits) * B

    @property
    def q8_out(self):
        """dest wo: do the rows leave the launch as Q8_K blocks (otherwise: f32 rows and the quantiser launch)?"""
        if self.dest != "wo":
            return False
        if self.form == "LIST":
            return self.dq == 1 and self.G % 2 == 0
        return self.form == "MMA" and self.NH % 2 == 0 and self.n_splits > 1 and rows_combine_applies(self.T, self.NH, self.n_splits)

    @property
    def expect_counters(self):
        """(nf_list_chains, nf_mma_chains) delta of one graph."""
        return {"LIST": (1, 0), "MMA": (0, 1), "DENSE": (0, 0)}[self.form]


def _counts(xs):
    return "counts:" + ",".join(str(x) for x in xs)


def _ladder(T, part, parts):
    """The part-th share of the count ladder for a batch of T tokens, filled up with counts next to the scratch trip and between the rungs."""
    own = list(LADDER[part::parts])
    fill = [15, 16, 17, 100, 300, 700, 2, 31, 33]
    assert len(own) <= T
    return _counts(own + fill[: T - len(own)])


def _cases():
    C, F16, F32 = Case, L.F16, L.F32
    out = [
        # the count ladder, once per slice count dq (rows_per 128 / 64 / 32 / 16; RB 16 / 8 / 8 / 4), on both sides of the G <= 4 choice at dq = 1
        C("ladder_dq1_g4", "LIST", 32, 8, 24, 4096, (_ladder(24, 0, 1),)),
        C("ladder_dq1_g8_f16", "LIST", 64, 8, 24, 4096, (_ladder(24, 0, 1),), mtype=F16),
        C("ladder_dq2_g5_a", "LIST", 40, 8, 12, 4096, (_ladder(12, 0, 2),)),
        C("ladder_dq2_g5_b", "LIST", 40, 8, 12, 4096, (_ladder(12, 1, 2),), mtype=F16),
        C("ladder_dq4_g3_a", "LIST", 24, 8, 10, 4096, (_ladder(10, 0, 2),), mtype=F16),
        C("ladder_dq4_g3_b", "LIST", 24, 8, 10, 4096, (_ladder(10, 1, 2),)),
        C("ladder_dq8_g6_a", "LIST", 24, 4, 10, 4096, (_ladder(10, 0, 2),)),
        C("ladder_dq8_g6_b", "LIST", 24, 4, 10, 4096, (_ladder(10, 1, 2),), mtype=F16),
        # list layouts at dq = 1 and at most 512 cells: the group form (runs = one 16-byte load, the rest gathered)
        C("layouts_dq1_g2", "LIST", 16, 8, 24, 2048, LAYOUTS),
        C("layouts_dq1_g7_f16", "LIST", 56, 8, 24, 2048, LAYOUTS, mtype=F16),
        # the remaining group sizes, token counts and destinations
        C("g1_dq1_kqv", "LIST", 8, 8, 24, 2048, ("np", "partial", _counts([513, 600, 1024, 1025] + [40 + 9 * t for t in range(20)])), dest="kqv"),
        C("g2_t32_kqv_f16", "LIST", 16, 8, 32, 1024, ("np", "stride", "run_odd"), mtype=F16, dest="kqv"),
        C("g8_dq1_scale", "LIST", 64, 8, 24, 2048, ("np", "groups64", _counts([513, 777, 1024] + [64 + 8 * t for t in range(21)])), scale=0.05),
        C("g1_t6_dq4", "LIST", 8, 8, 6, 2048, (_counts([1, 9, 256, 513, 1024, 1100]), "np")),
        C("g3_t2_nkv2_dq8", "LIST", 6, 2, 2, 2048, (_counts([600, 1100]), "np", _counts([0, 1024]))),
        C("g4_t2_nkv1_dq8_f16", "LIST", 4, 1, 2, 1024, (_counts([257, 8]), "np"), mtype=F16),
        C("g4_dq2_kqv", "LIST", 32, 8, 12, 2048, (_counts([7, 64, 255, 512, 513, 1024, 1025, 1300, 3, 90, 400, 800]), "np"), dest="kqv"),
        # ... into a quantised mat-mul: Q8_K blocks from the launch (G even, dq = 1), f32 rows + quantiser launch (G odd; dq > 1)
        C("wo_g4_dq1", "LIST", 32, 8, 24, 2048, ("np", "run_aligned", "stride", _counts([513, 1024, 1025] + [8 + 20 * t for t in range(21)])), dest="wo"),
        C("wo_g2_dq1_f16", "LIST", 16, 8, 24, 1024, ("np", "partial"), mtype=F16, dest="wo"),
        C("wo_g3_dq1", "LIST", 24, 8, 24, 2048, ("np", "run_odd", _counts([513, 1024, 1025] + [8 + 20 * t for t in range(21)])), dest="wo"),
        C("wo_g4_dq2", "LIST", 32, 8, 12, 2048, ("np", _counts([9, 64, 257, 512, 513, 1024, 1025, 1200, 5, 77, 300, 640])), dest="wo"),
        # shapes the list form refuses: the dense kernels, counters unchanged
        C("refused_g16", "DENSE", 32, 2, 4, 256, ("np",)),
        C("refused_d64", "DENSE", 8, 2, 4, 256, ("np",), HD=64),
        C("refused_nkv_mod4", "DENSE", 8, 2, 4, 258, ("np",)),
        C("refused_average_row", "DENSE", 8, 2, 2, 2052, (_counts([600, 1100]),)),
        C("refused_named_long_row", "DENSE", 8, 2, 4, 2048, (_counts([1100, 50, 60, 70]),), mask_name="KQ_mask"),
        # the matrix-core form: T edges x n_kv edges (one split; a short last split; a split without a tile) x G x destinations
        C("mma_t33_kv64_g1", "MMA", 8, 8, 33, 64, MMA_FAMILIES),
        C("mma_t64_kv72_g2_kqv", "MMA", 8, 4, 64, 72, MMA_FAMILIES, dest="kqv"),
        C("mma_t65_kv256_g4", "MMA", 16, 4, 65, 256, MMA_FAMILIES),
        C("mma_t128_kv520_g8_wo", "MMA", 16, 2, 128, 520, MMA_FAMILIES, dest="wo"),
        C("mma_t129_kv1032_g2", "MMA", 16, 8, 129, 1032, MMA_FAMILIES),
        C("mma_t160_kv1600_g4_wo", "MMA", 16, 4, 160, 1600, MMA_FAMILIES, dest="wo"),
        C("mma_t33_kv1600_g8_kqv", "MMA", 8, 1, 33, 1600, MMA_FAMILIES, dest="kqv"),
        C("mma_t64_kv1032_g1_wo_rows", "MMA", 8, 8, 64, 1032, ("full", "causal_end", "tile_states"), dest="wo"),
        C("mma_t40_kv520_g2_scale", "MMA", 8, 4, 40, 520, ("full", "blockdiag", "tile_states"), scale=0.05),
        # an f16 mask at 33 tokens: neither form
        C("refused_mma_f16_mask", "DENSE", 8, 4, 33, 256, ("full", "causal_end"), mtype=L.F16),
    ]
    return out


CASES = _cases()
GROUP_CASES = ("layouts_dq1_g2", "layouts_dq1_g7_f16")  # run once more with GGML_MI355X_NF_GROUPS=0 in a child process


# ------------------------------------------------------------------------------------------ visibility families
def _run_len(t):
    return 8 * (1 + (5 * t) % 64)


def list_cells(case, fam, t):
    """The cells token t sees in family fam (ascending)."""
    T, nkv = case.T, case.nkv
    ar = np.arange
    if fam.startswith("counts:"):
        n = [int(x) for x in fam[7:].split(",")][t]
        if n == 0:
            return ar(0)
        r, o = n // 2, (37 * t + 3) % 61   # a run (odd and even starts) and, one cell further on, every second or third cell
        s = 3 if (t % 2 and o + r + 1 + 3 * (n - r) < nkv) else 2
        cells = np.concatenate([o + ar(r), o + r + 1 + s * ar(n - r)])
        assert cells[-1] < nkv, (case.id, fam, t)
        return cells
    if fam == "np":  # a -np batch: the prompt's run, then every T-th cell (test_non_flash_attention_chain's pattern)
        run = (nkv // 2) // T // 4 * 4
        return np.concatenate([ar(t * run, (t + 1) * run), ar(T * run + t, nkv, T)])
    if fam in ("run_aligned", "run_odd", "run_shift"):
        n = min(_run_len(t), nkv // 2)
        start = 8 * ((11 * t) % ((nkv - n - 8) // 8)) + {"run_aligned": 0, "run_odd": 1 + 2 * (t % 4), "run_shift": (4, 2, 6)[t % 3]}[fam]
        return ar(start, start + n)
    if fam == "stride":
        n = 1 + (13 * t) % min(512, (nkv - t) // T)
        return t + T * ar(n)
    if fam == "partial":  # the last group holds 1 .. 7 entries; some tokens have nothing but that group
        n = 8 * ((3 * t) % 40) + 1 + t % 7
        start = 16 * t
        return ar(start, start + n)
    if fam == "groups64":  # exactly 512 cells: 64 groups, one ballot
        n = 512
        if t % 3 == 0:
            return ar(8 * t, 8 * t + n)
        if t % 3 == 1:
            return np.concatenate([ar(2 * t, 2 * t + n // 2), 2 * t + 1 + n // 2 + 2 * ar(n // 2)])
        return t + 3 * ar(n)
    if fam == "run_to_end":  # ends on the cache's last cell: aligned runs (the last 16-byte load ends on the row's end) and odd starts
        n = 8 * (1 + t) + (3 if t % 2 else 0)
        return ar(nkv - n, nkv)
    if fam == "run_from_zero":
        return ar(0, 5 + 21 * t)
    raise ValueError(fam)


def family_vis(case, fam):
    """-> (vis [T, nkv] bool, values [T, nkv] f16 or None: the mask value of a visible cell where it is not +0.0)."""
    T, nkv = case.T, case.nkv
    B = nf_constants()["bkv"]
    t = np.arange(T)[:, None]
    cell = np.arange(nkv)[None, :]
    if fam == "full":
        return np.ones((T, nkv), bool), None
    if fam == "causal_end":  # a prompt chunk at the end of the context
        return cell < nkv - T + t + 1, None
    if fam == "blockdiag":
        nseq = 5
        bounds = [(int(round(i * nkv / nseq)) | 1) if 0 < i < nseq else (0 if i == 0 else nkv) for i in range(nseq + 1)]
        lo = np.array([bounds[i % nseq] for i in range(T)])[:, None]
        hi = np.array([bounds[i % nseq + 1] - (i % 7) for i in range(T)])[:, None]
        return (cell >= lo) & (cell < hi), None
    if fam == "interleaved":
        return (cell % 3 == t % 3) & (cell < nkv - (t % 3)), None
    if fam == "tile_states":
        # whole (32-query, 64-cell) tiles in state 0 (nothing), 2 (every value +0.0) and 1: one visible cell, -0.0 on every second cell, all but one cell
        st = (cell // B + t // nf_constants()["scan_q"] + 1) % 3
        sub = t % 3
        one = cell == (cell // B) * B + (7 * t) % B
        vis = (st == 2) | ((st == 1) & (((sub == 0) & one) | ((sub == 1) & (cell % 2 == 0)) | ((sub == 2) & (cell % B != 17))))
        vals = np.zeros((T, nkv), np.float16)
        vals[(st == 1) & (sub == 1) & vis] = -0.0
        if case.dest != "wo":  # (a NaN row has no Q8_K image)
            vis[5] = False     # one token sees nothing
        return vis, vals
    vis = np.zeros((T, nkv), bool)
    for tt in range(T):
        vis[tt, list_cells(case, fam, tt)] = True
    return vis, None


# ------------------------------------------------------------------------------------------ edge sets
def list_edges(n):
    """Entry indices into a list of n cells: the first and last entries, both sides of the ends of groups of eight (the first, the second, the 63rd / 64th, the last), of
    every 256-thread stride, of the group form's 512, of NF_CAP, and of the first and last 16-cell trip of the scratch path."""
    c = nf_constants()
    g, th, trip = c["group"], c["threads"], c["scratch_trip"]
    s = {0, 1, n - 2, n - 1}
    for b in (g, 2 * g, c["group_max"] - g, c["group_max"], c["cap"], (n - 1) // g * g, trip, (n - 1) // trip * trip) + tuple(range(th, n + 1, th)):
        s |= {b - 1, b}
    s |= {c["group_max"] + 1, c["cap"] + 1, g + 1}
    return sorted(e for e in s if 0 <= e < n)


def list_pair_ends(n):
    """Boundaries b with entries b - 1 and b on its two sides."""
    c = nf_constants()
    s = {c["group"], c["scratch_trip"], c["threads"], c["group_max"], c["cap"], (n - 1) // c["group"] * c["group"], (n - 1) // c["threads"] * c["threads"]}
    return sorted(b for b in s if 1 <= b < n)


def mma_edges(case):
    """Cells: 0, n_kv - 1, both sides of every 64-cell tile end, of the first and of the last split boundary."""
    B, per, n = nf_constants()["bkv"], case.per, case.nkv
    last = (n - 1) // per * per
    s = {0, n - 1, per - 1, per, per + 1, last - 1, last}
    for b in range(B, n, B):
        s |= {b - 1, b}
    return sorted(e for e in s if 0 <= e < n)


def mma_pair_ends(case):
    B, per, n = nf_constants()["bkv"], case.per, case.nkv
    s = {B, (n - 1) // B * B, per, (n - 1) // per * per}
    return sorted(b for b in s if 1 <= b < n)


def edge_family(case):
    return case.families[0]


def token_lists(case, fam=None):
    """The cells each token may see in the case's edge family — its list in the list form; every cell of the family in the matrix-core form."""
    vis, _ = family_vis(case, fam or edge_family(case))
    return [np.flatnonzero(vis[t]) for t in range(case.T)]


def edges_of(case, n):
    """Witness positions (indices into a token's n cells)."""
    if n == 0:
        return []
    return mma_edges(case) if case.form == "MMA" or (case.form == "DENSE" and case.T > nf_constants()["t_max"]) else list_edges(n)


def pair_ends_of(case, n):
    if n < 2:
        return []
    return mma_pair_ends(case) if case.form == "MMA" else list_pair_ends(n)


# ------------------------------------------------------------------------------------------ the float64 twin
def _soft_pv(w, V, cells=None):
    """w [R, n] logits (-inf: masked), V [nkv or n, HD] (cells: the rows of V the n logits belong to) -> (out [R, HD], den [R]) with ggml-cpu's steps: max,
    e = exp(w - max), sum, the zero / NaN-sum guard, p = e / sum rounded to f16 (the second MUL_MAT rounds its src1), V^T.p."""
    R, n = w.shape
    if n == 0:  # expf(-inf - -inf) in every cell of the CPU's row
        return np.full((R, V.shape[1]), np.nan), np.full(R, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = w.max(axis=1, keepdims=True)
        e = np.exp(w - m)
        s = e.sum(axis=1, keepdims=True)
        g = np.where(np.isnan(s) | (s == 0.0), -np.inf, s)
        p = e * (1.0 / g)
        big = ~(p <= 2.0 ** -25)  # (at or below half the smallest f16 subnormal the rounding gives 0; NaN stays.  numpy's conversion of such values is slow)
        p16 = np.zeros_like(p)
        p16[big] = p[big].astype(np.float16).astype(np.float64)
        p = p16
        if cells is None:
            out = p @ V
        else:  # (only the rows that carry weight: a witness probe leaves one or two)
            nz = (p != 0).any(axis=0)
            out = p[:, nz] @ V[cells[nz]]
        out = np.where(np.isnan(s), np.nan, out)
    return out, s[:, 0]


def twin_lists(q, Kd, Vd, lists, mvals, scale, scores=None):
    """The chain over explicit lists: token t reads cells lists[t] (repeats allowed: the mutation checks use that) with mask values mvals[t].
    q [T, NH, HD] f32, Kd / Vd [nkv, NKV, HD] float64; scores: q16 . K of every cell [T, NH, nkv], where the caller has them.  -> (out [T, NH, HD], den [T, NH])."""
    T, NH, D = q.shape
    NKV = Kd.shape[1]
    G = NH // NKV
    q16 = q.astype(np.float16).astype(np.float64)
    out, den = np.zeros((T, NH, D)), np.zeros((T, NH))
    zero_q = not q.any()
    for t in range(T):
        cells = np.asarray(lists[t], np.int64)
        mv = np.asarray(mvals[t], np.float64)
        for k in range(NKV):
            hs = slice(k * G, (k + 1) * G)
            s = np.zeros((G, len(cells))) if zero_q else (scores[t, hs][:, cells] if scores is not None else q16[t, hs] @ Kd[cells, k].T)
            out[t, hs], den[t, hs] = _soft_pv(s * scale + mv[None, :], Vd[:, k], cells)
    return out, den


def full_scores(q, Kd):
    """q16 . K of every cell, without scale: [T, NH, nkv]."""
    T, NH, D = q.shape
    nkv, NKV, _ = Kd.shape
    G = NH // NKV
    q16 = q.astype(np.float16).astype(np.float64)
    return np.concatenate([(q16[:, k * G:(k + 1) * G].reshape(T * G, D) @ Kd[:, k].T).reshape(T, G, nkv) for k in range(NKV)], axis=1)


def twin(q, Kd, Vd, mask, scale, scores=None):
    """The chain as ggml-cpu computes it (attn_nf.hip's header): q rounded to f16, w = s * scale + mask, max, e = exp(w - max), the sum with the zero / NaN guard,
    p = e / sum rounded to f16, V^T.p; a token that sees nothing gives a NaN row.  mask [>= T, nkv] f16 / f32 (-inf: masked).  -> (out [T, NH, HD], den [T, NH])."""
    T, NH, D = q.shape
    nkv, NKV, _ = Kd.shape
    G = NH // NKV
    mk = np.asarray(mask[:T], np.float64)
    vis = mk != -np.inf
    if vis.sum() < 0.25 * vis.size:  # (sparse rows: only the listed cells)
        lists = [np.flatnonzero(vis[t]) for t in range(T)]
        return twin_lists(q, Kd, Vd, lists, [mk[t, lists[t]] for t in range(T)], scale, scores)
    out, den = np.zeros((T, NH, D)), np.zeros((T, NH))
    if scores is None and q.any():
        scores = full_scores(q, Kd)
    nothing = np.repeat(~vis.any(axis=1), G)
    for k in range(NKV):
        hs = slice(k * G, (k + 1) * G)
        s = np.zeros((T * G, nkv)) if scores is None else scores[:, hs].reshape(T * G, nkv)
        o, d = _soft_pv(s * scale + np.repeat(mk, G, axis=0), Vd[:, k])
        o[nothing] = np.nan
        d[nothing] = np.nan
        out[:, hs], den[:, hs] = o.reshape(T, G, D), d.reshape(T, G)
    return out, den


# ------------------------------------------------------------------------------------------ probe inputs
_KV = {}


def _kv_base(nkv, EK):
    """One random K and V (V on a grid of 1 / 64: sums of two rows are exact) per cache shape, shared by every case and probe:
    -> (K f16 [nkv, EK], V f16 [nkv, EK], V transposed [EK, nkv], K float64, V float64)."""
    if (nkv, EK) not in _KV:
        rng = np.random.default_rng(nkv * 131 + EK)
        k = rng.standard_normal((nkv, EK), np.float32).astype(np.float16)
        v = (np.round(rng.standard_normal((nkv, EK), np.float32) * 64.0) / 64.0).astype(np.float16)
        _KV[(nkv, EK)] = (k, v, np.ascontiguousarray(v.T), k.astype(np.float64), v.astype(np.float64))
    return _KV[(nkv, EK)]


def _rng(case, salt):
    return np.random.default_rng((sum((i + 1) * ord(ch) for i, ch in enumerate(case.id)) * 1000003 + salt) % (1 << 32))


def _vt(v16):
    return np.ascontiguousarray(v16.T)  # the transposed cache [n_embd_v, n_ctx]


def indicator_probes(case, families=None):
    """-> [Probe]: every family x pattern A, and pattern B wherever it keeps every residue at or below half of each token's cells."""
    nkv, D = case.nkv, case.HD
    k16, _, _, k64, _ = _kv_base(nkv, case.NKV * D)
    Kd = k64.reshape(nkv, case.NKV, D)
    q = np.zeros((case.T, case.NH, D), np.float32)
    cells = np.arange(nkv)
    out = []
    for fam in families or case.families:
        vis, vals = family_vis(case, fam)
        nv = vis.sum(axis=1)
        for pn, res in (("A", cells % D), ("B", (cells // D) % D)):
            cnt = np.stack([np.bincount(res[vis[t]], minlength=D) for t in range(case.T)])
            if not bool(np.all((2 * cnt.max(axis=1) <= nv) | (nv <= 1))):
                assert pn == "B", f"{case.id} {fam}: pattern A puts more than half of a token's visible cells on one residue"
                continue
            vx = np.zeros((nkv, case.NKV, D), np.float16)
            vx[cells, :, res] = 1.0
            mask = mask_of(vis, vals)
            exp, den = twin(q, Kd, vx.astype(np.float64), mask, case.sc)
            out.append(Probe(f"indicator_{pn}_{fam}", q, k16, _vt(vx.reshape(nkv, -1)), Kd, vx.astype(np.float64), mask, None, exp, den))
    return out


def _witness_q(case, Kd, wit, vis, cls):
    """q [T, NH, HD]: head h of token t asks with gamma * K[wit[t, h]] of its KV head; gamma doubled until every witness leads every other visible score (cells with
    the same K row, cls, apart) by MARGIN_NATS.  wit < 0: the token sees nothing and asks with zeros.  -> (q, gamma, margin, scores [T, NH, nkv])"""
    gamma = 12.0
    w = np.maximum(wit, 0)
    kvh = (np.arange(case.NH) // case.G)[None, :]
    others = vis[:, None, :] & (cls[None, None, :] != cls[w][:, :, None])
    shared = bool((wit == wit[:, :1]).all())
    while True:
        q = (gamma * Kd[w, kvh]).astype(np.float32)
        q[wit < 0] = 0
        # (pairs and 'last' masks give every head of a token the same witness: one head's scores per KV head, repeated)
        S = np.repeat(full_scores(q[:, :: case.G], Kd), case.G, axis=1) if shared else full_scores(q, Kd)
        top = np.take_along_axis(S, w[:, :, None], axis=2)[:, :, 0]
        rest = np.where(others, S, -np.inf).max(axis=2)
        margin = float(np.min(np.where(wit >= 0, (top - rest) * case.sc, np.inf)))
        if margin >= MARGIN_NATS:
            return q, gamma, margin, S
        gamma *= 2.0
        assert gamma < 1000, case.id


def _finish(case, name, q, k_run, vt, Kd, Vd, vis, wit, part, cls, gamma, margin, S, own):
    mask = mask_of(vis)
    exp, den = twin(q, Kd, Vd, mask, case.sc, S)
    p = Probe(name, q, k_run, vt, Kd, Vd, mask, None, exp, den, vmax=float(np.abs(Vd).max()))
    tied = (vis[:, None, :] & (cls[None, None, :] == cls[np.maximum(wit, 0)][:, :, None])).sum(axis=2)
    p.margin, p.gamma, p.witness, p.scores = margin, gamma, (wit, part), S
    p.residual = float(np.nanmax(np.where(wit >= 0, den - tied, 0.0)))  # the weight every cell but the witness (pair) holds
    p.own = own
    return p


def witness_probes(case, pair=False):
    """-> [Probe].
    witness: in run r head h of token t takes entry (r * NH + h + t) of the token's own edge set as its witness — every entry of every token's edge set is some head's
    witness ('mid': the token sees its whole list); and once per run every head of token t takes the token's entry (r * NH + t) with the prefix that ends on it ('last').
    pair: the witness on entry b - 1 and a cell with the same K row on entry b, for every boundary b of every token's boundary set.  The K cache is shared between the
    tokens of a run, so a pair that would touch another token's cells waits for a later run; tokens without a pair in a run keep a single witness.
    p.own lists the (token, slot) a probe carries at their own position."""
    T, NH, nkv, D = case.T, case.NH, case.nkv, case.HD
    k16, _, vt, k64, v64 = _kv_base(nkv, case.NKV * D)
    Vd = v64.reshape(nkv, case.NKV, D)
    lists = token_lists(case)
    sets = [(pair_ends_of if pair else edges_of)(case, len(c)) for c in lists]
    vis_mid, _ = family_vis(case, edge_family(case))
    first = np.array([int(c[0]) if len(c) else -1 for c in lists])
    cellno = np.arange(nkv)[None, :]
    out = []
    if not pair:
        Kd = k64.reshape(nkv, case.NKV, D)
        cls = np.arange(nkv)
        for run in range(max(1, -(-max(len(s) for s in sets) // NH))):
            for variant in ("mid", "last"):
                wit = np.repeat(first[:, None], NH, axis=1)
                own = []
                for t in range(T):
                    if not sets[t]:
                        continue
                    for h in range(NH if variant == "mid" else 1):
                        slot = (run * NH + h + t) % len(sets[t])
                        wit[t, h if variant == "mid" else slice(None)] = lists[t][sets[t][slot]]
                        own.append((t, slot))
                vis = vis_mid & (cellno <= wit[:, :1]) if variant == "last" else vis_mid
                q, gamma, margin, S = _witness_q(case, Kd, wit, vis, cls)
                out.append(_finish(case, f"witness_{variant}_run{run}", q, k16, vt, Kd, Vd, vis, wit, np.full(T, -1), cls, gamma, margin, S, sorted(set(own))))
        return out
    todo = {(t, s) for t in range(T) for s in range(len(sets[t]))}
    run = 0
    while todo:
        k_run, Kd, cls = k16.copy(), k64.reshape(nkv, case.NKV, D).copy(), np.arange(nkv)
        wit1, part, own = first.copy(), np.full(T, -1), []
        want = {}
        for t in range(T):
            mine = sorted(s for tt, s in todo if tt == t)
            if mine:
                want[t] = mine[(run + t) % len(mine)]
                wit1[t] = lists[t][sets[t][want[t]] - 1]
        taken = set(int(wit1[t]) for t in want)  # the witness of a pair keeps its own K row (the token with the highest one is never refused: every run carries a pair)
        sources, partners = {}, set()
        for t, s in want.items():
            a, b = int(wit1[t]), int(lists[t][sets[t][s]])
            if sources.get(a) == b or (a not in sources and a not in partners and b not in partners and b not in sources and b not in taken):
                sources[a] = b
                partners.add(b)
                k_run[b] = k_run[a]
                Kd[b] = Kd[a]
                cls[b] = a
                part[t] = b
                own.append((t, s))
        assert own, case.id
        todo -= set(own)
        wit = np.repeat(wit1[:, None], NH, axis=1)
        for variant in ("mid", "last"):
            vis = vis_mid & (cellno <= np.maximum(wit1, part)[:, None]) if variant == "last" else vis_mid
            q, gamma, margin, S = _witness_q(case, Kd, wit, vis, cls)
            out.append(_finish(case, f"pair_{variant}_run{run}", q, k_run, vt, Kd, Vd, vis, wit, part, cls, gamma, margin, S, sorted(own)))
        run += 1
        assert run < 64, case.id
    return out


def random_probe(case):
    """Random data over the edge family; finite mask values -1.5 and 0.75 (exact in f16) in some 64-cell blocks, -0.0 in the first."""
    rng = _rng(case, 9)
    nkv, D = case.nkv, case.HD
    k16, _, vt, k64, v64 = _kv_base(nkv, case.NKV * D)
    Kd, Vd = k64.reshape(nkv, case.NKV, D), v64.reshape(nkv, case.NKV, D)
    q = rng.standard_normal((case.T, case.NH, D)).astype(np.float32)
    vis, _ = family_vis(case, edge_family(case))
    if case.form == "MMA":  # (every tile state next to the finite values)
        vis = vis & family_vis(case, "tile_states")[0] | family_vis(case, "causal_end")[0] & (np.arange(case.T)[:, None] % 4 == 1)
    vals = np.zeros(vis.shape, np.float16)
    cell = np.arange(nkv)
    tile = cell // nf_constants()["bkv"]
    vals[:, tile % 3 == 1] = -1.5
    vals[:, (tile % 3 == 2) & (cell % 7 == 0)] = 0.75
    vals[:, (tile == 0) & (cell % 5 == 0)] = -0.0
    mask = mask_of(vis, vals)
    exp, den = twin(q, Kd, Vd, mask, case.sc)
    return Probe("random", q, k16, vt, Kd, Vd, mask, None, exp, den, vmax=float(np.abs(Vd).max()))


# ------------------------------------------------------------------------------------------ running a probe
_READOUT = {}


def run_probe(case, p, target, H, n_threads=4):
    """The chain exactly as test_non_flash_attention_chain builds it, on `target` ('oracle' or the backend) -> [T, NH, HD] float32."""
    import harness as T_
    import probes as PR
    D, NH, NKV, T, nkv = case.HD, case.NH, case.NKV, case.T, case.nkv
    EK, E = NKV * D, NH * D
    if case.dest == "wo" and E not in _READOUT:
        _READOUT[E] = PR.readout_weight(L.Q4_K, E)
    TP = p.mask.shape[0]
    mask = p.mask.astype(np.float32) if case.mtype == L.F32 else p.mask

    def build(g):
        qq = H.ggml_permute(g.ctx, g.new(L.F32, [D, NH, T], p.q), 0, 2, 1, 3)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [EK, nkv], p.kraw), D, nkv, NKV, EK * 2, D * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [nkv, EK], p.vraw), nkv, D, NKV, nkv * 2, nkv * 2 * D, 0)
        kq = H.ggml_mul_mat(g.ctx, k, qq)
        sm = H.ggml_soft_max_ext(g.ctx, kq, g.new(case.mtype, [nkv, TP], mask, name=case.mask_name or None), float(case.sc), 0.0)
        kqv = H.ggml_mul_mat(g.ctx, v, sm)
        cur = H.ggml_cont_2d(g.ctx, H.ggml_permute(g.ctx, kqv, 0, 2, 1, 3), D * NH, T)
        if case.dest == "kqv":
            return [cur, kqv]
        if case.dest == "wo":
            return H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [E, E], _READOUT[E]), cur)
        return cur

    outs = T_.run_case(build, target, n_threads)
    got = np.asarray(outs[0], np.float32).reshape(T, NH, D)
    if case.dest == "kqv":  # kqv's own layout [D, T, NH]; the copy made from it must hold the same bits
        own = np.asarray(outs[1], np.float32).reshape(NH, T, D).transpose(1, 0, 2)
        assert np.array_equal(own.view(np.uint32), got.view(np.uint32)), f"{case.id} {p.name}: kqv and its CONT copy differ"
    return got


_FORM_SEEN = set()


def run_counted(case, p, backend, H):
    """run_probe on the backend -> (result, None or a sentence on the form that ran).  The counters move while graph_compute walks the graph; a graph the backend
    recognises (same nodes, shapes and addresses as an earlier run) is replayed from its capture without a walk — that is accepted only after a counted run of the same
    case, whose launches the capture holds."""
    keys = ("nf_list_chains", "nf_mma_chains", "graph_launches")
    want = case.expect_counters
    if case.mask_name and (np.asarray(p.mask[: case.T], np.float32) != -np.inf).sum(axis=1).max() <= nf_constants()["named_row_max"]:
        want = (1, 0)  # (a named mask is refused for its longest row only: a probe that shortens the rows is the list form's again)
    c0 = [backend.stat(k) for k in keys]
    got = run_probe(case, p, backend, H)
    ran = tuple(backend.stat(k) - v for k, v in zip(keys, c0))
    if ran[:2] == want:
        _FORM_SEEN.add((case.id, want))
        return got, None
    if ran[:2] == (0, 0) and ran[2] == 1 and (case.id, want) in _FORM_SEEN:
        return got, None
    return got, f"{case.id} {p.name}: expected (list, matrix-core) chains {want}, ran {ran[:2]} with {ran[2]} graph launches"


def check_probe(case, p, got, quant_step=False):
    """fa_ref.check_probe with the NaN rows of tokens that see nothing compared first; -> the measured figure."""
    got = np.asarray(got, np.float64)
    nan_row = np.isnan(p.expect).all(axis=(1, 2))
    assert np.isnan(got[nan_row]).all(), f"{case.id} {p.name}: a token that sees nothing must give the CPU's NaN row (tokens {np.flatnonzero(nan_row)})"
    assert not np.isnan(p.expect[~nan_row]).any()
    clean = dataclasses.replace(p, expect=np.where(nan_row[:, None, None], 0.0, p.expect), den=np.where(nan_row[:, None], 1.0, p.den))
    return FR.check_probe(case, clean, np.where(nan_row[:, None, None], 0.0, got), quant_step)


def nmse_rows(got, ref):
    """NMSE over the rows that are not NaN in the reference; the NaN rows must be NaN in both."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN rows differ"
    d = np.where(nan, 0.0, got - np.where(nan, 0.0, ref))
    return float((d * d).sum() / np.where(nan, 0.0, ref * ref).sum())
