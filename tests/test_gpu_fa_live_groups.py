"""k_fattn_dec128 requests only the LIVE row groups of a trip: a wave loads row group u of the trip at p0 only if its first row of that group, p0 + u * WV * RPW +
wave * RPW, lies before the split's end (list mode: before the list's end); a dead group loads nothing and its dot products and P.V terms are skipped.  What can
go wrong is a live cell that is no longer read, or registers nobody loaded that still reach a sum — so every case here puts a split's end at a chosen place
inside a trip (option fa_splits forces the split count, the cache length sets `per`) and compares with

  the CPU oracle's FLASH_ATTN_EXT at the gate test_flash_attn / test_flash_attn_q8_0_kv use for the same kernel form (nmse 1e-4 over an f16 cache, whose
      reference accumulates V in f16; 1e-6 over a q8_0 cache, where both sides do the same integer arithmetic), and
  the float64 twin of tests/fa_ref.py at test_flash_attn's gate for the f32-accumulating lane kernel (nmse 1e-9; f16 cache only — over q8_0 the kernel asks
      with ggml-cpu's 8-bit query, which the twin does not model).  With scores of order one, ONE missing or doubled cell among n moves the result by about
      1 / n of its size, nmse ~ 1 / n^2 >= 1.6e-6 at the largest cache used here (774 cells): three orders above this gate.

Shapes: one KV head x G query heads, one token, random K / V / Q, mask 0 over a prefix and -inf after it (the prefix ends inside the last split, so that split
has masked live cells, clamped rows and dead groups at once).  The constants (rows per wave-instruction, row groups, trip) come from fa_ref's parse of fattn.hip.
"""
import numpy as np
import pytest

import fa_ref as FR
import harness as T
import llama_box_amd as L
from model_util import Context, Model, greedy, preset

pytestmark = pytest.mark.gpu

ORACLE_GATE = {L.F16: 1e-4, L.Q8_0: 1e-6}
TWIN_GATE = 1e-9


def _case(G, nkv, splits, D=128, kv=L.F16, waves=8, nq=1, mode=0, tail="COMBINE"):
    return FR.Case(f"live_g{G}_n{nkv}_s{splits}", "DEC", mode, waves, tail, D, G, 1, nq, nkv, kv=kv, splits=splits)


def _data(case, seed, vis=None, n_vis=None):
    """Random Q / K / V and the prefix mask -> (q, kx, vx, mask)."""
    rng = np.random.default_rng(seed)
    kx = rng.standard_normal((case.nkv, case.NKV * case.HD)).astype(np.float16).astype(np.float32)
    vx = rng.standard_normal((case.nkv, case.NKV * case.HD)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((case.NH, case.nq, case.HD)).astype(np.float32)
    if vis is None:
        vis = np.zeros((case.nq, case.nkv), bool)
        vis[:, : (case.nkv if n_vis is None else n_vis)] = True
    return q, kx, vx, FR.mask_of(vis)


def _run(case, H, target, q, kraw, vraw, mask, tail_rows=None):
    """FLASH_ATTN_EXT through the C-ABI -> [nq, NH, HD] f32.  tail_rows [n, NKV * HD] (f16 cache): rows of the cache TENSOR behind the view's last cell."""
    HD, NH, NKV, nq, nkv = case.HD, case.NH, case.NKV, case.nq, case.nkv
    nctx = nkv + (0 if tail_rows is None else len(tail_rows))
    kc = kraw if tail_rows is None else np.concatenate([kraw, tail_rows])
    vc = vraw if tail_rows is None else np.concatenate([vraw, tail_rows])

    def build(g):
        tq = g.new(L.F32, [HD, nq, NH], q)
        rb, hb = FR.row_bytes(case.kv, NKV * HD), FR.row_bytes(case.kv, HD)
        k = H.ggml_view_3d(g.ctx, g.new(case.kv, [NKV * HD, nctx], kc), HD, nkv, NKV, rb, hb, 0)
        v = H.ggml_view_3d(g.ctx, g.new(case.kv, [NKV * HD, nctx], vc), HD, nkv, NKV, rb, hb, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, mask.shape[0]], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    out = T.run_case(build, target, T.host_threads(8) if target == "oracle" else 4)[0]
    return np.asarray(out, np.float32).reshape(nq, NH, HD)


def _gpu(backend, H, case, q, kraw, vraw, mask, tail_rows=None):
    backend.set_option("fa_splits", case.splits)
    try:
        got = _run(case, H, backend, q, kraw, vraw, mask, tail_rows)
        ran = backend.stat("fa_form")
    finally:
        backend.set_option("fa_splits", 0)
    assert ran == case.form, f"{case.id}: expected form [{FR.form_name(case.form)}], ran [{FR.form_name(ran)}]"
    return got


def _check(backend, H, plog, case, seed, vis=None, n_vis=None):
    q, kx, vx, mask = _data(case, seed, vis, n_vis)
    kraw, Kd = FR.make_cache(case, kx)
    vraw, Vd = FR.make_cache(case, vx)
    got = _gpu(backend, H, case, q, kraw, vraw, mask)
    ref = _run(case, H, "oracle", q, kraw, vraw, mask)
    e_o = T.nmse(got, ref)
    msg = f"fa_live {case.id} D={case.HD} kv={case.kv} per={case.per(case.nkv) if case.mode != 2 else '-'} trip={case.trip}: nmse vs oracle {e_o:.3e}"
    assert np.isfinite(got).all()
    if case.kv == L.F16:
        e_t = T.nmse(got, FR.twin(q, Kd, Vd, mask, 1.0 / np.sqrt(case.HD))[0])
        plog(msg + f", vs float64 twin {e_t:.3e}")
        assert e_t <= TWIN_GATE
    else:
        plog(msg)
    assert e_o <= ORACLE_GATE[case.kv]
    return got


def _per_cases():
    """(G, per, splits, nkv): three splits, the last one cell short, so that ceil(nkv / 3) is exactly `per`; per = 1: one cell per split."""
    out = []
    for G in (4, 2, 8):
        trip = FR.trip_len(128, G, 8)
        for per in (1, 31, 32, 33, 64, 96, 97, 127, 128, 129, trip + 1):  # (trip + 1: a second trip with ONE live row — 129 again at G = 4)
            if (G, per) not in [(g, p) for g, p, _, _ in out]:
                out.append((G, per, 3, 3 if per == 1 else 3 * per - 1))
    return out


@pytest.mark.parametrize("G,per,splits,nkv", _per_cases())
def test_split_end_inside_a_trip_eight_waves(backend, H, plog, G, per, splits, nkv):
    case = _case(G, nkv, splits)
    assert case.per(nkv) == per and case.trip == (16 // FR.gg(G)) * 32
    _check(backend, H, plog, case, 100 * G + per, n_vis=max(1, nkv - max(1, per // 3)))


def test_four_waves_q8_0_cache(backend, H, plog):
    """Four waves (a q8_0 cache), G = 4: trip 64, row group 16; per = 81 = a trip, one whole row group and one row."""
    case = _case(4, 3 * 81 - 1, 3, kv=L.Q8_0, waves=4)
    assert case.per(case.nkv) == 81 and case.trip == 64
    _check(backend, H, plog, case, 7, n_vis=case.nkv - 30)


def test_head_dim_64(backend, H, plog):
    """Eight-lane rows: eight rows per wave-instruction, trip 128 = two row groups of 64 at G = 4; per = 65: the second group has one live row."""
    case = _case(4, 3 * 65 - 1, 3, D=64)
    assert case.per(case.nkv) == 65 and case.trip == 128
    _check(backend, H, plog, case, 8, n_vis=case.nkv - 20)


def test_list_form_partly_live_and_dead_groups(backend, H, plog):
    """Position lists, two tokens whose visible cells interleave; 85 entries each = a trip of 64, one whole row group of 16, five entries of the next, two dead groups."""
    case = _case(4, 172, 1, waves=4, nq=2, mode=2, tail="NONE")
    assert case.trip == 64
    cell = np.arange(case.nkv)[None, :]
    vis = (cell % 2 == np.arange(2)[:, None]) & (cell < 170)
    assert (vis.sum(axis=1) == 85).all()
    _check(backend, H, plog, case, 9, vis=vis)


def test_splits_past_the_cache_leave_empty_records(backend, H, plog):
    """40 cells, 16 splits of 3: splits 14 and 15 begin past the cache: no trip, an empty record each, and the combine pass ignores them."""
    case = _case(4, 40, 16)
    assert case.per(case.nkv) * 14 >= case.nkv
    _check(backend, H, plog, case, 10, n_vis=37)


def test_unread_cells_may_hold_nan(backend, H, plog):
    """Cells no split may read hold NaN: the rows of the cache TENSOR behind the view's last cell (where a next split's range would lie: the last split is one
    cell short, so its clamped rows and its dead groups sit right in front of them), K and V; and, inside the view, the K rows of split 1's masked cells (a
    masked score is replaced, never used — V rows of cells a split DOES read cannot be poisoned: 0 * NaN, before this change as after).  Finite, and bit for bit
    the result of the run with finite values in those places."""
    case = _case(4, 3 * 97 - 1, 3)
    per, n_vis = case.per(case.nkv), 97 + 40
    q, kx, vx, mask = _data(case, 11, n_vis=n_vis)
    kraw, vraw = FR.make_cache(case, kx)[0], FR.make_cache(case, vx)[0]
    rng = np.random.default_rng(12)
    clean_tail = rng.standard_normal((case.trip, case.HD)).astype(np.float16)
    clean = _gpu(backend, H, case, q, kraw, vraw, mask, clean_tail)
    kpoison = kraw.copy()
    kpoison[n_vis : 2 * per] = np.nan  # (split 1 = cells [97, 194): visible up to 137, NaN keys behind)
    got = _gpu(backend, H, case, q, kpoison, vraw, mask, np.full_like(clean_tail, np.nan))
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), clean.view(np.uint32))
    assert T.nmse(got, _run(case, H, "oracle", q, kraw, vraw, mask)) <= ORACLE_GATE[L.F16]


@pytest.mark.parametrize("extra", [1, 33, 64])
def test_appended_masked_cells_change_no_bit(backend, H, plog, extra):
    """Four splits of exactly one trip each against the same cells with `extra` masked cells appended to EVERY split (per = trip + extra: each split keeps its
    live cells and gains a second trip of masked cells — one live row, a group and a row, two groups — and dead groups behind them).  A masked cell has
    probability 0 and rescales by 2^0: every record, hence the result, keeps its bits."""
    G, S = 4, 4
    trip = FR.trip_len(128, G, 8)
    a = _case(G, S * trip, S)
    b = _case(G, S * (trip + extra), S)
    assert a.per(a.nkv) == trip and b.per(b.nkv) == trip + extra
    q, kx, vx, mask_a = _data(a, 13)
    rng = np.random.default_rng(14)
    kb = rng.standard_normal((b.nkv, a.HD)).astype(np.float16).astype(np.float32)
    vb = rng.standard_normal((b.nkv, a.HD)).astype(np.float16).astype(np.float32)
    vis = np.zeros((1, b.nkv), bool)
    for s in range(S):
        lo = s * (trip + extra)
        kb[lo : lo + trip], vb[lo : lo + trip] = kx[s * trip : (s + 1) * trip], vx[s * trip : (s + 1) * trip]
        vis[0, lo : lo + trip] = True
    one = _gpu(backend, H, a, q, kx.astype(np.float16), vx.astype(np.float16), mask_a)
    two = _gpu(backend, H, b, q, kb.astype(np.float16), vb.astype(np.float16), FR.mask_of(vis))
    plog(f"fa_live appended masked cells: per {trip} -> {trip + extra}, {np.count_nonzero(one.view(np.uint32) != two.view(np.uint32))} values differ")
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))


def test_hipgraph_replay_with_dead_groups_is_bit_identical_to_eager(backend, H, plog):
    """Decode steps of a small model (two query heads per KV head: eight row groups of 32 cells) with three forced splits over the 256-cell view: per = 86,
    five dead groups in every workgroup — replayed graphs and eager launches give the same logits bit for bit."""
    hp = preset("test-llama", n_head=4, n_head_kv=2, n_embd=512, n_embd_head=128)
    mg = Model(hp, 99, backend.buft)
    prompt = [1, 5, 9, 300, 17, 42, 99, 7]
    outs = {}
    try:
        backend.set_option("fa_splits", 3)
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            c = Context(mg, backend=backend, flash_attn=1)
            l0 = backend.stat("graph_launches")
            ids, rows = greedy(c, prompt, 24)
            outs[mode] = (ids, np.stack(rows), backend.stat("graph_launches") - l0, backend.stat("fa_form"))
            c.free()
    finally:
        backend.set_option("graphs", 1)
        backend.set_option("fa_splits", 0)
        mg.free()
    plog(f"fa_live hipGraph launches with graphs=1: {outs[1][2]}, with graphs=0: {outs[0][2]}; form [{FR.form_name(outs[1][3])}]")
    assert outs[1][3] == outs[0][3] and (outs[1][3] & 15) == FR.fa_constants()["form"]["FA_FORM_K_DEC"] and ((outs[1][3] >> 6) & 15) == 8
    assert outs[1][2] >= 10 and outs[0][2] == 0
    assert outs[1][0] == outs[0][0]
    assert np.array_equal(outs[1][1].view(np.uint32), outs[0][1].view(np.uint32))
