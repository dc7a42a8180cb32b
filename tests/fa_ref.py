"""FLASH_ATTN_EXT cell accounting: a float64 twin, three probes whose expected result is known exactly, masks and edge positions derived from the
kernels' constants, and the table of kernel forms (shared by test_fa_ref_host.py on the CPU and test_gpu_fa_cells.py on the GPU).

Every kernel form of csrc/fattn.hip / csrc/fattn_mma.hip decides WHICH cache cells it reads with its own arithmetic (trip lengths, split lengths, clamps,
list entries past the count, trip masks, tile states).  The probes make one wrong cell an order-one error, whatever that arithmetic is:

  indicator  Q = 0, V[c, d] = 1 where c % D == d (pattern A) or (c // D) % D == d (pattern B): every visible score is exactly 0, every weight equal, so
             out * denominator is the NUMBER of visible cells per residue.  Gate |out - twin| * den <= 0.01: f32 rounding gives at most n_vis * 2^-22
             (1e-3 at 4224 cells); one missing / doubled cell moves a residue by (n_vis - count_r) / (n_vis -+ 1) >= 0.5 while no residue holds more than
             half of a token's visible cells (asserted on the inputs; a token with ONE visible cell returns that V row or is wrong by 1).
  witness    K, V random f16; every head of token t asks with gamma * K[c_t] (its own KV head), gamma doubled until the float64 margin between the witness
             score and every other visible score is >= 60 nats: the others weigh <= n_kv * e^-60 < 1e-9 together, the result is the V row of the witness.
             Gate max |out - V[c_t]| <= 1e-6 * max |V| (f32 rounding plus the asserted residual weight).
  pair       two witnesses with identical K rows in different trips / tiles / splits: (V[c1] + V[c2]) / 2, same gate.  With sinks the sink of head h is set
             6 nats below that head's witness score: it takes e^-6 / (2 + e^-6) = 1.2e-3 of the weight (1000 x the gate when dropped, doubled or taken
             from another head) and an f32 score error delta moves the result by 1.2e-3 * delta, below the gate for delta up to 1e-3.
No gate here is taken from a kernel's output."""
import os
import re
from dataclasses import dataclass

import numpy as np

import llama_box_amd as L

CSRC = os.path.join(L.REPO, "llama_box_amd", "csrc")
INDICATOR_GATE = 0.01
WITNESS_GATE = 1e-6   # times max |V|
MARGIN_NATS = 60.0
SINK_BELOW = 6.0


# ------------------------------------------------------------------------------------------ constants parsed from the kernels
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(text, pattern, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, f"{what}: pattern {pattern!r} matches {len(m)} times — the expression moved, edit tests/fa_ref.py: fa_constants"
    return m[0]


_CONST = None


def fa_constants():
    """The constants that decide which cells a form reads and which form runs, parsed from the expressions in fattn.hip / fattn_mma.hip / kernels.h.
    If an expression is rewritten, the one pattern below that names it is the line to edit (and EDGE_TABLE in test_fa_ref_host.py says what moved)."""
    global _CONST
    if _CONST is not None:
        return _CONST
    fa, mma, kh = _src("fattn.hip"), _src("fattn_mma.hip"), _src("kernels.h")
    c = {}
    m = _one(fa, r"constexpr int LPR = D / (\d+), RPW = (\d+) / LPR, NG = LPR / G;", "lane geometry of k_fattn_dec128")
    c["dims_per_lane"], c["wave"] = int(m[0]), int(m[1])
    _one(fa, r"constexpr int (TRIP = NG \* WV \* RPW);", "trip formula of k_fattn_dec128")
    _one(fa, r"fa_gg\(const int64_t G\) \{ (return G <= 2 \? 2 : \(G <= 4 \? 4 : 8\);) \}", "template form of a head group")
    c["split_ng"] = int(_one(fa, r"constexpr int NG = (\d+); ", "row groups of k_fattn_split"))
    _one(fa, r"for \(; p0 < kv1; (p0 \+= NG \* 4 \* RPW)\)", "trip of k_fattn_split")
    bkv = set(re.findall(r"constexpr int BKV = (\d+);", mma))
    assert len(bkv) == 1, bkv
    c["bkv"] = int(bkv.pop())
    c["scan_q"] = int(_one(mma, r"const int qi = qt \* (\d+) \+ r;", "query tile of k_fattn_vis_scan"))
    m = _one(mma, r"const int nw = geo\.n_q >= (\d+) \? (\d+) : (\d+);", "workgroup size of k_fattn_mma")
    c["wg128_min_q"], c["nw_big"], c["nw_small"] = int(m[0]), int(m[1]), int(m[2])
    qpw = set(re.findall(r"dim3 grid\(\(unsigned\) \(\(geo\.n_q \+ nw \* (\d+) - 1\)", mma))  # (the flash kernel and the non-flash chain's: the same tile)
    assert len(qpw) == 1, qpw
    c["q_per_wave"] = int(qpw.pop())
    c["pos_scan_pass"] = int(_one(fa, r"for \(int c0 = 0; c0 < n_kv; c0 \+= (\d+)\) \{\n        const int pp = c0 \+ 4 \* tid;", "pass of k_fattn_pos_scan"))
    c["mma_min_q"] = int(_one(mma, r"atoi\(getenv\(\"GGML_MI355X_FA_MMA_MIN_Q\"\)\)\) : (\d+);", "fattn_mma_min_q"))
    c["rows_min"] = int(_one(fa, r"n_rows >= (\d+) && n_rows <", "fattn_combine_rows_applies, rows"))
    m = _one(fa, r"n_splits >= (\d+) && n_splits <= (\d+) && n_rows", "fattn_combine_rows_applies, splits")
    c["rows_splits"] = (int(m[0]), int(m[1]))
    c["skip_trips"] = int(_one(fa, r"per <= (\d+) \* 16 \* \(16 / fa_gg\(G\)\)", "trip bound of the skip form"))
    c["skip_round"] = int(_one(fa, r"geo\.n_splits \+ 63\) / (\d+) \* 64;", "split rounding of the skip form"))
    c["fat_trip"] = int(_one(fa, r"const int64_t trip = (\d+) \* \(16 / fa_gg\(G\)\);", "fat trip"))
    c["fat_max"] = int(_one(fa, r"int64_t splits = std::min<int64_t>\((\d+), trips\);", "fat split bound"))
    c["dec_want"] = int(_one(fa, r"int64_t want = \((\d+) \+ groups - 1\) / groups;", "decode chooser, workgroups"))
    c["dec_len"] = int(_one(fa, r"max_by_len = std::max<int64_t>\(1, n_kv / (\d+)\);", "decode chooser, length"))
    m = _one(fa, r"want \* groups > (\d+)\) want = std::max<int64_t>\(1, (\d+) / groups\);", "decode chooser, f16 cap")
    c["dec_cap"] = int(m[0])
    assert m[0] == m[1]
    c["mma_want"] = int(_one(mma, r"int64_t want = \((\d+) \+ wgs - 1\) / wgs;", "matrix-core chooser, workgroups"))
    m = _one(mma, r"std::min<int64_t>\(want, std::min<int64_t>\((\d+), tiles / (\d+)\)\)", "matrix-core chooser, tiles")
    c["mma_max"], c["mma_tiles_per"] = int(m[0]), int(m[1])
    c["form"] = {k: int(v) for k, v in re.findall(r"(FA_FORM_[A-Z0-9_]+) = (\d+)", kh)}
    _one(kh, r"return (kernel \| \(mode << 4\) \| \(waves << 6\) \| \(kv << 10\) \| \(\(D == 128 \? 1 : 0\) << 12\) \| \(tail << 13\);)", "fa_form_code")
    _CONST = c
    return c


def gg(G):
    return 2 if G <= 2 else (4 if G <= 4 else 8)


def trip_len(D, G, waves, kernel="dec"):
    """Cells (or list entries) per workgroup trip."""
    c = fa_constants()
    lpr = D // c["dims_per_lane"]
    rpw = c["wave"] // lpr
    if kernel == "split":
        return c["split_ng"] * 4 * rpw
    return (lpr // gg(G)) * waves * rpw


def fat_splits(n_kv, G):
    c = fa_constants()
    trip = c["fat_trip"] * (16 // gg(G))
    trips = -(-n_kv // trip)
    splits = min(c["fat_max"], trips)
    per = -(-trips // splits)
    return -(-trips // per), per * trip


def decode_splits(n_kv, groups, f16=True):
    c = fa_constants()
    want = -(-c["dec_want"] // groups)
    want = max(1, min(want, max(1, n_kv // c["dec_len"]), 64))
    if f16 and want * groups > c["dec_cap"]:
        want = max(1, c["dec_cap"] // groups)
    return want


def mma_splits(nq, NH, n_kv):
    c = fa_constants()
    qt = c["nw_big"] * c["q_per_wave"] if nq >= c["wg128_min_q"] else c["nw_small"] * c["q_per_wave"]
    wgs = -(-nq // qt) * NH
    tiles = -(-n_kv // c["bkv"])
    return max(1, min(-(-c["mma_want"] // wgs), c["mma_max"], tiles // c["mma_tiles_per"]))


def form(kernel, mode=0, waves=4, kv="F16", D=128, tail="NONE"):
    f = fa_constants()["form"]
    return f["FA_FORM_K_" + kernel] | (mode << 4) | (waves << 6) | (f["FA_FORM_KV_" + kv] << 10) | ((1 if D == 128 else 0) << 12) | (f["FA_FORM_TAIL_" + tail] << 13)


def form_name(code):
    f = fa_constants()["form"]
    inv = lambda pre, v: next((k[len(pre):] for k, x in f.items() if k.startswith(pre) and x == v), str(v))
    return (f"{inv('FA_FORM_K_', code & 15)} mode={(code >> 4) & 3} waves={(code >> 6) & 15} kv={inv('FA_FORM_KV_', (code >> 10) & 3)} "
            f"D={128 if (code >> 12) & 1 else 64} tail={inv('FA_FORM_TAIL_', (code >> 13) & 7)}")


# ------------------------------------------------------------------------------------------ the cases: one or more per kernel form
@dataclass(frozen=True)
class Case:
    id: str
    kernel: str        # SPLIT / DEC / MMA
    mode: int          # DEC: 0 plain, 1 skip, 2 list; MMA: 1 = with tile states
    waves: int
    tail: str          # NONE / COMBINE / COMBINE_ROWS / SELF_MERGE / MERGE2 / FAT
    HD: int
    NH: int
    NKV: int
    nq: int
    nkv: int
    kv: int = L.F16
    splits: int = 1    # option fa_splits (0: the dispatcher's own chooser)
    masked: bool = True
    sinks: bool = False
    alibi: float = 0.0
    self_merge: bool = False
    wo: bool = False   # the result goes through a reshape into a quantised read-out matrix (the fat form)
    sparse_name: bool = False  # the mask is called KQ_mask: its upload statistics send a sparse 33 .. 256-token batch to the position lists
    kvform: str = ""   # cache kind of the form code when it is not the cache type's own (Q8_IMAGE)

    @property
    def G(self):
        return self.NH // self.NKV

    @property
    def form(self):
        kvf = self.kvform or {L.F16: "F16", L.Q8_0: "Q8_0", L.Q4_0: "BLOCK"}[self.kv]
        return form(self.kernel, self.mode, self.waves, kvf, self.HD, self.tail)

    @property
    def n_splits(self):
        if self.wo:
            return fat_splits(self.nkv, self.G)[0]
        if self.splits:
            return self.splits
        if self.kernel == "MMA":
            return mma_splits(self.nq, self.NH, self.nkv)
        assert self.nq == 1
        return decode_splits(self.nkv, self.NKV, self.kv == L.F16)

    @property
    def trip(self):
        if self.kernel == "MMA":
            return fa_constants()["bkv"]
        return trip_len(self.HD, self.G, self.waves, "split" if self.kernel == "SPLIT" else "dec")

    def per(self, n=None):
        """Cells (list mode: entries, of a list n long) per split."""
        c = fa_constants()
        S = self.n_splits
        if self.wo:  # (the launcher divides the cells evenly: never more than the whole trips fattn_fat_splits counted)
            assert -(-self.nkv // S) <= fat_splits(self.nkv, self.G)[1]
            return -(-self.nkv // S)
        if self.kernel == "MMA":
            return -(-(-(-self.nkv // c["bkv"])) // S) * c["bkv"]
        if self.mode == 2:
            trips = -(-n // self.trip)
            return -(-trips // S) * self.trip
        per = -(-self.nkv // S)
        return -(-per // c["skip_round"]) * c["skip_round"] if self.mode == 1 else per


def _cases():
    F, Q8, Q4 = L.F16, L.Q8_0, L.Q4_0
    C = Case
    return [
        # generic k_fattn_split: ALiBi at head size 128 (soft-capping bounds every score, so no witness can lead by 60 nats); head size 64 with 2 .. 32 tokens and no mask
        C("split_d128_alibi", "SPLIT", 0, 4, "COMBINE", 128, 4, 2, 2, 260, splits=2, alibi=8.0),
        C("split_d64_nomask", "SPLIT", 0, 4, "NONE", 64, 4, 2, 5, 67, masked=False),
        C("split_d64_odd_kv", "SPLIT", 0, 4, "COMBINE", 64, 8, 1, 2, 333, splits=3),
        # k_fattn_dec128, plain mode, four waves
        C("plain4_d128_g2_nomask", "DEC", 0, 4, "NONE", 128, 4, 2, 1, 333, masked=False),
        C("plain4_d128_g8_sinks", "DEC", 0, 4, "NONE", 128, 8, 1, 1, 516, sinks=True),
        C("plain4_d128_g3_tokens", "DEC", 0, 4, "COMBINE", 128, 6, 2, 5, 1028, splits=3, masked=False),
        C("plain4_d64_g1_nomask", "DEC", 0, 4, "NONE", 64, 2, 2, 1, 67, masked=False),   # one real head in the two-head template
        C("plain4_q8_0", "DEC", 0, 4, "COMBINE", 128, 8, 2, 1, 516, kv=Q8, splits=3),
        C("plain4_q4_0", "DEC", 0, 4, "COMBINE", 128, 4, 2, 1, 260, kv=Q4, splits=2),
        # ... eight waves: one token, f16 cache, >= 2 splits
        C("wide8_d128_g2", "DEC", 0, 8, "COMBINE", 128, 4, 2, 1, 2052, splits=5),
        C("wide8_d128_g1_sinks", "DEC", 0, 8, "COMBINE", 128, 2, 2, 1, 516, splits=3, sinks=True),
        C("wide8_d64_g8_chooser", "DEC", 0, 8, "COMBINE", 64, 8, 1, 1, 4100, splits=0),
        C("wide8_d64_g3", "DEC", 0, 8, "COMBINE", 64, 6, 2, 1, 516, splits=3),             # three real heads in the four-head template
        # ... fat form: the records stay for the prologue of the quantised wo mat-vec
        C("fat_one_trip_splits", "DEC", 0, 8, "FAT", 128, 2, 1, 1, 2052, splits=0, wo=True),
        C("fat_two_trip_splits", "DEC", 0, 8, "FAT", 128, 2, 1, 1, 4100, splits=0, wo=True),
        # ... list mode
        # (query heads per KV head below the template's — 1 in the two-head form, 3 in the four-head form: surplus slots ask with a zero query, records and outputs
        #  are indexed by the real group size — at both head sizes, in list, skip and self-merging forms too)
        C("list_d128_g3_one", "DEC", 2, 4, "NONE", 128, 6, 2, 5, 516),
        C("list_d128_g8_splits", "DEC", 2, 4, "COMBINE", 128, 8, 1, 32, 1028, splits=3),
        C("list_d64_g4_one", "DEC", 2, 4, "NONE", 64, 8, 2, 2, 260),
        C("list_d64_g1_one", "DEC", 2, 4, "NONE", 64, 2, 2, 5, 260),
        C("list_d64_g3_splits", "DEC", 2, 4, "COMBINE", 64, 6, 2, 5, 2052, splits=4),
        C("list_q8_0", "DEC", 2, 4, "COMBINE", 128, 8, 2, 5, 516, kv=Q8, splits=2),
        C("list_q4_0", "DEC", 2, 4, "NONE", 128, 4, 2, 2, 1028, kv=Q4),
        C("list_sparse_40", "DEC", 2, 4, "COMBINE", 128, 4, 2, 40, 2052, splits=2, sparse_name=True),
        # ... skip mode: where lists do not apply — 33 .. 64 tokens with sinks (the matrix-core kernel takes none) and >= 2 splits
        C("skip_d128_g3_sinks", "DEC", 1, 4, "COMBINE", 128, 6, 2, 40, 1028, splits=3, sinks=True),
        C("skip_q8_0_sinks", "DEC", 1, 4, "COMBINE", 128, 8, 2, 33, 516, kv=Q8, splits=2, sinks=True),
        # matrix cores
        C("mma_d128_33", "MMA", 1, 2, "NONE", 128, 4, 2, 33, 260),
        C("mma_d64_40_splits", "MMA", 1, 2, "COMBINE", 64, 4, 2, 40, 1028, splits=3),
        C("mma_d128_264_nomask", "MMA", 0, 4, "NONE", 128, 2, 1, 264, 516, masked=False),
        C("mma_d128_rows", "MMA", 1, 2, "COMBINE_ROWS", 128, 32, 8, 64, 1028, splits=2),
        C("mma_d64_264_chooser", "MMA", 1, 4, "COMBINE", 64, 2, 1, 264, 4224, splits=0),
        C("mma_q8_0_image", "MMA", 1, 2, "COMBINE", 128, 4, 2, 33, 516, kv=Q8, splits=2, kvform="Q8_IMAGE"),
        # option fa_self_merge on the forms above
        C("merge2_wide8", "DEC", 0, 8, "MERGE2", 128, 4, 2, 1, 2052, splits=5, self_merge=True),
        C("self_merge_list_g1", "DEC", 2, 4, "SELF_MERGE", 128, 2, 2, 32, 1028, splits=3, self_merge=True),
        C("self_merge_skip", "DEC", 1, 4, "SELF_MERGE", 128, 4, 2, 40, 1028, splits=3, sinks=True, self_merge=True),
    ]


CASES = _cases()
# forms that sit behind an environment switch read once at start-up: listed, not run
NOT_RUN = {
    "list mode on eight waves": "GGML_MI355X_FA_LIST_WV8=1",
    "plain four-wave kernel for several masked tokens and >= 2 splits with n_kv % 4 == 0": "GGML_MI355X_FA_SKIP=0",
    "generic kernel for multi-head attention": "GGML_MI355X_FA_G_MIN=2",
}


# ------------------------------------------------------------------------------------------ the float64 twin
def twin(q, Kd, Vd, mask, scale, sinks=None, alibi=0.0):
    """Exact FLASH_ATTN_EXT: q [NH, nq, HD] f32 (rounded to f16 as the op does), Kd / Vd [nkv, NKV, HD] float64, mask [>= nq, nkv] f16 or None.
    -> (out [nq, NH, HD], denominator [nq, NH] relative to the row maximum, scores [nq, NH, nkv] without the mask)."""
    NH, nq, HD = q.shape
    nkv, NKV, _ = Kd.shape
    G = NH // NKV
    q16 = q.astype(np.float16).astype(np.float64)
    mk = mask[:nq].astype(np.float64) if mask is not None else np.zeros((nq, nkv))
    out, den, sc = np.zeros((nq, NH, HD)), np.zeros((nq, NH)), np.zeros((nq, NH, nkv))
    n2 = 1 << int(np.floor(np.log2(NH)))
    for h in range(NH):
        slope = 1.0
        if alibi > 0:
            slope = (2.0 ** (-alibi / n2)) ** (h + 1) if h < n2 else (2.0 ** (-alibi / 2 / n2)) ** (2 * (h - n2) + 1)
        s0 = q16[h] @ Kd[:, h // G].T * scale
        sc[:, h] = s0
        with np.errstate(invalid="ignore", divide="ignore"):
            s = s0 + slope * mk
            m = s.max(axis=1)
            if sinks is not None:
                m = np.maximum(m, float(sinks[h]))
            p = np.exp(s - m[:, None])
            d = p.sum(axis=1) + (np.exp(float(sinks[h]) - m) if sinks is not None else 0.0)
            out[:, h] = (p @ Vd[:, h // G]) / d[:, None]
        den[:, h] = d
    return out, den, sc


# ------------------------------------------------------------------------------------------ caches
def row_bytes(t, n):
    return n // L.TYPE_BLCK[t] * L.TYPE_SIZE[t]


def make_cache(case, x, image=False):
    """x [nkv, NKV * HD] f32 -> (bytes / array for the cache tensor, its values float64 [nkv, NKV, HD] as the kernel form sees them)."""
    import ctypes as C
    import harness as T
    nkv = x.shape[0]
    if case.kv == L.F16:
        raw = x.astype(np.float16)
        return raw, raw.astype(np.float64).reshape(nkv, case.NKV, case.HD)
    lib = T.oracle()
    src = np.ascontiguousarray(x, np.float32)
    raw = np.zeros(row_bytes(case.kv, src.size), np.uint8)
    lib.oracle_quantize_row(case.kv, src.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p), src.size)
    back = np.zeros(src.size, np.float32)
    lib.oracle_dequantize_row(case.kv, raw.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p), src.size)
    if case.kvform == "Q8_IMAGE":  # the matrix-core kernel reads the f16 image of the blocks: d * q rounded to f16 once
        back = back.astype(np.float16).astype(np.float32)
    return raw.reshape(nkv, -1), back.astype(np.float64).reshape(nkv, case.NKV, case.HD)


# ------------------------------------------------------------------------------------------ masks
def mask_of(vis, values=None):
    """vis [nq, nkv] bool -> the F16 mask ggml pads to 64 rows (padding rows see nothing); values: finite mask values for visible cells."""
    nq, nkv = vis.shape
    m = np.full(((nq + 63) // 64 * 64, nkv), -np.inf, np.float16)
    m[:nq][vis] = 0
    if values is not None:
        m[:nq][vis] = values[vis]
    return m


def family_masks(case, indicator=True):
    """[(name, vis [nq, nkv] bool or None)]: the mask families of the indicator probe."""
    nq, nkv = case.nq, case.nkv
    c = fa_constants()
    B = c["bkv"]
    t = np.arange(nq)[:, None]
    cell = np.arange(nkv)[None, :]
    if not case.masked:
        return [("none", None)]
    out = []
    nseq = min(max(nq, 2), 5)
    bounds = [(int(round(i * nkv / nseq)) | 1) if 0 < i < nseq else (0 if i == 0 else nkv) for i in range(nseq + 1)]  # odd: aligned neither to 4 nor to 64
    lo = np.array([bounds[i % nseq] for i in range(nq)])[:, None]
    hi = np.array([bounds[i % nseq + 1] - (i % 7) for i in range(nq)])[:, None]
    out.append(("blockdiag", (cell >= lo) & (cell < hi)))
    out.append(("interleaved", (cell % 3 == t % 3) & (cell < nkv - (t % 3))))
    out.append(("single_first", (cell == 0) & (t >= 0)))
    out.append(("single_last", (cell == nkv - 1) & (t >= 0)))
    tiles = nkv // B
    if tiles >= 2:
        kt = 1 + t % (tiles - 1)
        out.append(("second_half", (cell >= kt * B + B // 2) & (cell < kt * B + B)))
        k0 = (t % (tiles - 1)) * B
        out.append(("zero_tile_next_to_one_inf", (cell >= k0) & (cell < k0 + 2 * B) & (cell != k0 + B + 17 + t % 5)))
    if nkv % B == 4:
        out.append(("ragged_last_tile_visible", np.ones((nq, nkv), bool)))
        out.append(("last_tile_only", (cell >= nkv - 4) & (t >= 0)))
    per = case.per(nkv)
    if case.n_splits > 1 and per < nkv:
        out.append(("first_split_only", (cell < per - (t % 3)) & (t >= 0)))  # every other split empty
    if case.wo and indicator:  # read through the wo mat-vec's Q8_K activation the indicator is used up to 2048 visible cells: one cell is then still 16 half-steps of amax / 254
        out = [f for f in out if f[1].sum(axis=1).max() <= 2048]
    if case.sparse_name:  # (denser masks are not this form's: their upload statistics send the batch to the matrix cores)
        out = [f for f in out if f[1].mean() <= 0.2]
    return out


def edge_positions(n, T, per):
    """Positions in [0, n): 0, 1, both sides of the first trip end, both sides of the first and the last split boundary, n - 2, n - 1."""
    last = (n - 1) // per * per
    s = {0, 1, T - 1, T, T + 1, per - 1, per, per + 1, last - 1, last, n - 2, n - 1}
    return sorted(p for p in s if 0 <= p < n)


def mma_positions(case):
    B = fa_constants()["bkv"]
    per = case.per()
    last = (case.nkv - 1) // B * B
    s = {0, B - 1, B, B + 1, 2 * B - 1, per - 1, per, per + 1, (case.nkv - 1) // per * per - 1, (case.nkv - 1) // per * per, last - 1, last, case.nkv - 2, case.nkv - 1}
    return sorted(p for p in s if 0 <= p < case.nkv)


def token_cells(case, t):
    """List mode: the scattered cells token t may see (its position list); the other forms: every cell."""
    if case.kernel == "DEC" and case.mode == 2:
        nseq = 3 if not case.sparse_name else 8
        return np.flatnonzero((np.arange(case.nkv) % nseq == t % nseq) & (np.arange(case.nkv) >= (t % 5)))
    return np.arange(case.nkv)


def edges_of(case, t=0):
    """Witness positions of token t: indices into token_cells(case, t)."""
    n = len(token_cells(case, t))
    if case.kernel == "MMA":
        return mma_positions(case)
    return edge_positions(n, case.trip, case.per(n))


# ------------------------------------------------------------------------------------------ probe inputs
@dataclass
class Probe:
    name: str
    q: np.ndarray
    kraw: np.ndarray
    vraw: np.ndarray
    Kd: np.ndarray
    Vd: np.ndarray
    mask: object
    sinks: object
    expect: np.ndarray   # [nq, NH, HD] float64
    den: object = None   # indicator: the twin's denominator [nq, NH]
    vmax: float = 1.0
    margin: float = 0.0  # witness / pair: nats between the witness and the best other visible score, the gamma that gave it, the cells, the others' total weight
    gamma: float = 0.0
    witness: object = None
    residual: float = 0.0
    own: object = None


def _rng(case, salt):
    return np.random.default_rng((sum((i + 1) * ord(ch) for i, ch in enumerate(case.id)) * 1000003 + salt) % (1 << 32))


def _kv_random(case, rng):
    x = rng.standard_normal((case.nkv, case.NKV * case.HD)).astype(np.float16).astype(np.float32)
    y = rng.standard_normal((case.nkv, case.NKV * case.HD)).astype(np.float16).astype(np.float32)
    return x, y


def indicator_probes(case):
    """-> [Probe]: every mask family x pattern A, and pattern B wherever it keeps every residue at or below half of each token's visible cells."""
    rng = _rng(case, 1)
    kx, _ = _kv_random(case, rng)
    kraw, Kd = make_cache(case, kx)
    q = np.zeros((case.NH, case.nq, case.HD), np.float32)
    D, nkv = case.HD, case.nkv
    cells = np.arange(nkv)
    pats = {"A": cells % D, "B": (cells // D) % D}
    sinks = np.zeros(case.NH, np.float32) if case.sinks else None  # (a sink at the score of every cell: one more unit in the denominator)
    out = []
    for fam, vis in family_masks(case):
        v = vis if vis is not None else np.ones((case.nq, nkv), bool)
        for pn, res in pats.items():
            cnt = np.stack([np.bincount(res[v[t]], minlength=D) for t in range(case.nq)])  # [nq, D]
            nv = v.sum(axis=1)
            ok = bool(np.all((2 * cnt.max(axis=1) <= nv) | (nv == 1)))
            if not ok:
                assert pn == "B", f"{case.id} {fam}: pattern A puts more than half of a token's visible cells on one residue"
                continue
            vx = np.zeros((nkv, case.NKV, D), np.float32)
            vx[cells, :, res] = 1.0
            vraw, Vd = make_cache(case, vx.reshape(nkv, -1))
            mask = mask_of(vis) if vis is not None else None
            exp, den, _ = twin(q, Kd, Vd, mask, 1.0 / np.sqrt(D), sinks, case.alibi)
            out.append(Probe(f"indicator_{pn}_{fam}", q, kraw, vraw, Kd, Vd, mask, sinks, exp, den))
    return out


def _witness_q(case, Kd, cells_of_tok, vis, scale):
    """q [NH, nq, HD] = gamma * K[witness of the token] per KV head, gamma doubled until the witness leads every other visible score by MARGIN_NATS."""
    G = case.G
    gamma = 12.0
    while True:
        q = np.zeros((case.NH, case.nq, case.HD), np.float32)
        for t in range(case.nq):
            for h in range(case.NH):
                q[h, t] = gamma * Kd[cells_of_tok[t], h // G]
        q16 = q.astype(np.float16).astype(np.float64)
        worst = np.inf
        for h in range(case.NH):
            s = q16[h] @ Kd[:, h // G].T * scale  # [nq, nkv]
            for t in range(case.nq):
                w = s[t, cells_of_tok[t]]
                others = vis[t].copy()
                others[s[t] == w] = False  # (the witness, and in the pair probe its twin row)
                if others.any():
                    worst = min(worst, w - s[t][others].max())
        if worst >= MARGIN_NATS:
            return q, gamma, worst
        gamma *= 2.0
        assert gamma < 1000


def witness_probes(case, pair=False):
    """-> [Probe].  Token t's witness sits on edge (run * nq + t) of its own edge set; two masks per run: 'last' (a causal prefix that ends on the witness) and
    'mid' (everything the token may see).  pair: a second cell with the same K row, on the far side of the next boundary (different trip / tile / split)."""
    rng = _rng(case, 2 + int(pair))
    kx, vx = _kv_random(case, rng)
    if pair:  # V on a grid of 1 / 64: the sum of two rows is exact in f16 too, so the CPU oracle's f16 accumulator of V can pass the same gate
        vx = np.round(vx * 64.0) / 64.0
    scale = 1.0 / np.sqrt(case.HD)
    n_edges = max(len(edges_of(case, t)) for t in range(case.nq))
    runs = -(-n_edges // case.nq)
    out = []
    # a run gives token t the edge slot (run * nq + t) of its edge set; a pair run whose neighbouring edges collide (the partner of edge 0 IS the split boundary)
    # leaves slots without a pair of their own: each of those gets a run in which every token takes that one slot
    queue = [(f"run{r}", None) for r in range(runs)]
    covered, n_slots = set(), len(edges_of(case, 0))
    while queue:
        tag, fixed = queue.pop(0)
        run = int(tag[3:]) if fixed is None else 0
        kx_run = kx.copy()
        wit, wit2, lists, slot = [], [], [], []
        for t in range(case.nq):
            cells, ed = token_cells(case, t), edges_of(case, t)
            slot.append((run * case.nq + t) % len(ed) if fixed is None else fixed % len(ed))
            e = ed[slot[-1]]
            lists.append(cells)
            wit.append(int(cells[e]))
            if pair:  # the partner: one trip and one split further on (wrapping), never the witness itself
                n = len(cells)
                e2 = (e + case.trip) % n if case.n_splits == 1 else (e + case.per(n)) % n
                if e2 == e:
                    e2 = (e + 1) % n
                wit2.append(int(cells[e2]))
        if pair:
            # K rows are shared between the tokens of a run: a pair (a, b) copies row a onto row b, so it stands only if neither cell takes part in another
            # pair (tokens with the SAME pair share it); a token whose pair collides uses token 0's, and `own` says which edge slots kept their own
            taken, pairs, own = set(), set(), set()
            for t in range(case.nq):
                ab = (wit[t], wit2[t])
                if ab not in pairs and (ab[0] == ab[1] or ab[0] in taken or ab[1] in taken):
                    wit[t], wit2[t] = ab = (wit[0], wit2[0])
                    if not (set(lists[t]) >= set(ab)):
                        lists[t] = np.union1d(lists[t], ab)
                else:
                    own.add(slot[t])
                pairs.add(ab)
                taken.update(ab)
                kx_run[ab[1]] = kx_run[ab[0]]
        kraw, Kd = make_cache(case, kx_run)
        vraw, Vd = make_cache(case, vx)
        for variant in ("last", "mid"):
            if not case.masked and variant == "last":
                continue
            vis = np.zeros((case.nq, case.nkv), bool)
            for t in range(case.nq):
                cells = lists[t]
                top = max(wit[t], wit2[t]) if pair else wit[t]
                vis[t, cells[cells <= top] if variant == "last" else cells] = True
            q, gamma, margin = _witness_q(case, Kd, wit, vis, scale)
            assert float(np.abs(q).max()) < 1000.0
            G = case.G
            exp = np.zeros((case.nq, case.NH, case.HD))
            sinks = None
            for t in range(case.nq):
                for h in range(case.NH):
                    exp[t, h] = (Vd[wit[t], h // G] + Vd[wit2[t], h // G]) / 2 if pair else Vd[wit[t], h // G]
            mask = mask_of(vis) if case.masked else None
            if case.sinks:
                _, _, sc = twin(q, Kd, Vd, None, scale)
                top = np.array([[sc[t, h, wit[t]] for h in range(case.NH)] for t in range(case.nq)])  # [nq, NH]
                if pair and case.kv == L.F16:  # (a quantised cache's lane kernels ask with an 8-bit query, as ggml-cpu does: the twin's f16 score is not theirs to 1e-3)
                    # the sink carries weight: SINK_BELOW nats under the lowest witness score of its head; the expectation comes from the twin
                    sinks = (top.min(axis=0) - SINK_BELOW).astype(np.float32)
                    exp = twin(q, Kd, Vd, mask, scale, sinks)[0]
                else:     # the sink is one more score the witness must lead by the margin
                    sinks = (top.min(axis=0) - MARGIN_NATS - 1.0).astype(np.float32)
            p = Probe(f"{'pair' if pair else 'witness'}_{variant}_{tag}", q, kraw, vraw, Kd, Vd, mask, sinks, exp, vmax=float(np.abs(Vd).max()))
            p.margin, p.gamma, p.witness = margin, gamma, (wit, wit2)
            p.own = sorted(own) if pair else sorted(set(slot))  # the edge slots (indices into the token's edge set) this run probes at their own position
            # the weight every cell but the witness (pair) holds, from the twin
            tw, den, _ = twin(q, Kd, Vd, mask, scale, None)
            p.residual = float(np.max(den - (2.0 if pair else 1.0)))
            out.append(p)
            covered.update(p.own)
        if pair and not queue and fixed is None:
            queue = [(f"slot{k}", k) for k in range(n_slots) if k not in covered]
    return out


def random_probe(case):
    """One random-data case: block-diagonal / interleaved visibility with finite mask values (-1.5, 0.75: exact in f16) in some tiles."""
    rng = _rng(case, 9)
    kx, vx = _kv_random(case, rng)
    kraw, Kd = make_cache(case, kx)
    vraw, Vd = make_cache(case, vx)
    q = rng.standard_normal((case.NH, case.nq, case.HD)).astype(np.float32)
    sinks = rng.standard_normal(case.NH).astype(np.float32) if case.sinks else None
    mask = None
    if case.masked:
        fams = dict(family_masks(case, indicator=False))
        vis = fams["blockdiag"] | fams["interleaved"] if not case.sparse_name else fams["blockdiag"]
        B = fa_constants()["bkv"]
        vals = np.zeros(vis.shape, np.float16)
        tile = np.arange(case.nkv) // B
        vals[:, tile % 3 == 1] = -1.5
        vals[:, (tile % 3 == 2) & (np.arange(case.nkv) % 7 == 0)] = 0.75
        mask = mask_of(vis, vals)
    exp = twin(q, Kd, Vd, mask, 1.0 / np.sqrt(case.HD), sinks, case.alibi)[0]
    return Probe("random", q, kraw, vraw, Kd, Vd, mask, sinks, exp, vmax=float(np.abs(Vd).max()))


# ------------------------------------------------------------------------------------------ running a probe
_READOUT = {}


def run_probe(case, p, target, H, n_threads=4):
    """FLASH_ATTN_EXT of the probe on `target` ('oracle' or the backend) -> [nq, NH, HD] float32 (the fat cases: read through a one-hot Q4_K matrix)."""
    import harness as T
    import probes as PR
    HD, NH, NKV, nq, nkv = case.HD, case.NH, case.NKV, case.nq, case.nkv
    E = NH * HD
    if case.wo and E not in _READOUT:
        _READOUT[E] = PR.readout_weight(L.Q4_K, E)

    def build(g):
        tq = g.new(L.F32, [HD, nq, NH], p.q)
        k = H.ggml_view_3d(g.ctx, g.new(case.kv, [NKV * HD, nkv], p.kraw), HD, nkv, NKV, row_bytes(case.kv, NKV * HD), row_bytes(case.kv, HD), 0)
        v = H.ggml_view_3d(g.ctx, g.new(case.kv, [NKV * HD, nkv], p.vraw), HD, nkv, NKV, row_bytes(case.kv, NKV * HD), row_bytes(case.kv, HD), 0)
        m = g.new(L.F16, [nkv, p.mask.shape[0]], p.mask, name="KQ_mask" if case.sparse_name else None) if p.mask is not None else None
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, m, 1.0 / np.sqrt(HD), case.alibi, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        if p.sinks is not None:
            H.ggml_flash_attn_ext_add_sinks(r, g.new(L.F32, [NH], p.sinks))
        if case.wo:
            return H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [E, E], _READOUT[E]), H.ggml_reshape_2d(g.ctx, r, E, nq))
        return r

    out = T.run_case(build, target, n_threads)[0]
    return np.asarray(out, np.float32).reshape(nq, NH, HD)


def check_probe(case, p, got, quant_step=False):
    """Asserts the probe's gate on `got` [nq, NH, HD]; -> the measured figure (for logs)."""
    got = got.astype(np.float64)
    if p.name.startswith("indicator"):
        dev = np.abs(got - p.expect) * p.den[:, :, None]
        gate = INDICATOR_GATE
        if quant_step:  # read through the Q8_K activation of the wo mat-vec: half a quantisation step of each 256-value block, in the same units
            amax = np.abs(p.expect.reshape(-1, 256)).max(axis=1)
            dev = (np.abs(got - p.expect).reshape(-1, 256) - (amax / 254)[:, None]).reshape(got.shape).clip(min=0) * p.den[:, :, None]
        worst = float(np.nanmax(np.where(np.isnan(dev), np.inf, dev)))
        assert worst <= gate, f"{case.id} {p.name}: |out - twin| * denominator = {worst:.3e} > {gate} at {np.unravel_index(np.argmax(np.where(np.isnan(dev), np.inf, dev)), dev.shape)} (token, head, residue)"
        return worst
    dev = np.abs(got - p.expect)
    if quant_step:
        amax = np.abs(p.expect.reshape(-1, 256)).max(axis=1)
        dev = (dev.reshape(-1, 256) - (amax / 254)[:, None]).reshape(got.shape).clip(min=0)
    dev = np.where(np.isnan(dev), np.inf, dev)
    worst = float(dev.max())
    gate = WITNESS_GATE * p.vmax
    assert worst <= gate, f"{case.id} {p.name}: max |out - expected| = {worst:.3e} > {gate:.3e} at {np.unravel_index(np.argmax(dev), dev.shape)} (token, head, dim); witnesses {getattr(p, 'witness', None)}"
    return worst
