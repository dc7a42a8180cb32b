"""FLASH_ATTN_EXT at K 576 / V 512 over one shared KV head (DeepSeek MLA with -fa; csrc/fattn_mla.hip): row mapping, KV tails and splits, mask forms, the
aliased and the separate V, a batch, and the refusals that stay.  Every computed case asserts supports_op first and the kernel form (stat "fa_form") afterwards.
The cache is a view into a wider, longer buffer whose other cells hold NaN, so an over-read shows.  Gates: the project's own (tests/fa_d256.py)."""
from collections import namedtuple

import numpy as np
import pytest

import fa_ref as FR
import harness as T
import llama_box_amd as L

pytestmark = pytest.mark.gpu

DK, DV, ROW, BEHIND = 576, 512, 640, 7  # head sizes; elements of a cache row (nb[1] = 1280 > 1152); NaN cells behind n_kv
ORACLE_F16 = 1e-4                       # tests/fa_d256.py
Case = namedtuple("Case", "NH nq nkv splits mask vsrc nb scale", defaults=(1, DK ** -0.5))  # vsrc: sep | a64 | a0 (a view of K at that element offset)


def make_inputs(c, seed=0):
    """-> q [nb, NH, nq, 576] f32, the K buffer and the separate V buffer [nkv + BEHIND, ROW] f16, mask [rows, nkv] f16 or None, and what the node sees: K, V float64."""
    rng = np.random.default_rng(1000 * c.NH + 10 * c.nkv + c.nq + seed)
    q = rng.standard_normal((c.nb, c.NH, c.nq, DK)).astype(np.float32)
    kbuf = np.full((c.nkv + BEHIND, ROW), np.nan, np.float16)
    kbuf[: c.nkv, :DK] = rng.standard_normal((c.nkv, DK))
    off = 0 if c.vsrc == "a0" else 64
    vbuf = np.full_like(kbuf, np.nan)
    vbuf[: c.nkv, :DV] = kbuf[: c.nkv, off : off + DV]  # the separate form on EQUAL data: the same values from a tensor of its own
    mask = None
    if c.mask != "none":
        mask = np.full(((c.nq + 63) // 64 * 64, c.nkv), -np.inf, np.float16)
        for t in range(c.nq):
            if c.mask == "causal":  # at the end of the context; every row keeps a visible cell
                mask[t, : max(1, c.nkv - c.nq + t + 1)] = 0
            else:                   # finite non-zero values
                mask[t] = rng.standard_normal(c.nkv) * 0.5
    return q, kbuf, vbuf, mask, kbuf[: c.nkv, :DK].astype(np.float64), vbuf[: c.nkv, :DV].astype(np.float64)


def twin(c, q, K, V, mask):
    """Q rounded to f16, K / V at their f16 values, scores * scale + mask, soft-max, P.V — float64.  -> [nb, nq, NH, 512]"""
    s = np.einsum("bhtd,cd->bthc", q.astype(np.float16).astype(np.float64), K) * c.scale
    if mask is not None:
        s = s + mask[None, : c.nq, None, :].astype(np.float64)
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)) @ V


def node(H, c, x=None, tk=L.F16, kvh=1, cap=0.0, bias=0.0, sinks=False):
    def build(g):
        q, kbuf, vbuf, mask = x[:4] if x else (None,) * 4
        tq = g.new(L.F32, [DK, c.nq, c.NH, c.nb], q)
        m = g.new(L.F16, [c.nkv, (c.nq + 63) // 64 * 64], mask) if c.mask != "none" else None
        if tk != L.F16 or kvh != 1:  # (refusals: plain tensors)
            k, v = g.new(tk, [DK, c.nkv, kvh]), g.new(tk, [DV, c.nkv, kvh])
        else:
            kc = g.new(L.F16, [ROW, c.nkv + BEHIND], kbuf)
            k = H.ggml_view_3d(g.ctx, kc, DK, c.nkv, 1, 2 * ROW, 2 * ROW * (c.nkv + BEHIND), 0)
            vc = g.new(L.F16, [ROW, c.nkv + BEHIND], vbuf) if c.vsrc == "sep" else kc
            v = H.ggml_view_3d(g.ctx, vc, DV, c.nkv, 1, 2 * ROW, 2 * ROW * (c.nkv + BEHIND), 128 if c.vsrc == "a64" else 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, m, c.scale, bias, cap)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        if sinks:
            H.ggml_flash_attn_ext_add_sinks(r, g.new(L.F32, [c.NH]))
        return r

    return build


def supported(backend, H, build):
    g = T.G(backend)
    try:
        return bool(H.ggml_backend_dev_supports_op(backend.dev, build(g)))
    finally:
        g.free()


def run_gpu(backend, H, c, x):
    assert supported(backend, H, node(H, c)), f"supports_op refuses FLASH_ATTN_EXT at K 576 / V 512: {c}"
    backend.set_option("fa_splits", c.splits)
    try:
        got = np.asarray(T.run_case(node(H, c, x), backend)[0], np.float32).reshape(c.nb, c.nq, c.NH, DV)
        form = backend.stat("fa_form")
    finally:
        backend.set_option("fa_splits", 0)
    assert form & 15 == FR.fa_constants()["form"]["FA_FORM_K_MLA"] and (form >> 4) & 3 == (0 if c.vsrc == "sep" else 1), f"{c}: ran [{FR.form_name(form)}]"
    return got


C = Case
CASES = [C(nh, nq, 70, 1, "causal", "a64") for nh in (128, 16, 5) for nq in (1, 3)] + [  # a full block / a block over two tokens / dead rows with an uneven span
    C(16, 40, 70, 1, "causal", "a64"),                                                    # ten workgroups; a tile wholly -inf for some rows of a block, visible for others
] + [C(16, 3, nkv, s, "causal", "sep" if s == 1 else "a64") for nkv in (1, 70, 262) for s in (1, 3)] + [  # tails, empty splits (1 and 70 cells at 3 splits)
    C(16, 3, 262, 3, "none", "a64"), C(16, 3, 262, 3, "bias", "a64"), C(16, 3, 262, 0, "causal", "a64"),  # mask forms; the chooser's own split count
    C(5, 3, 96, 1, "bias", "sep"),                                                        # whole tiles and 8-byte aligned mask rows: four mask values a load
    C(5, 3, 70, 1, "none", "sep"), C(5, 3, 70, 1, "causal", "a0"),                        # V sources (a64: above)
    C(16, 3, 70, 3, "causal", "a64", nb=2), C(16, 3, 70, 1, "causal", "a64", scale=192 ** -0.5),
]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(str(f) for f in c[:7]) + ("-s192" if c.scale != DK ** -0.5 else ""))
def test_flash_attn_mla(backend, H, plog, c):
    x = make_inputs(c)
    exact = twin(c, x[0], x[4], x[5], x[3])
    got = run_gpu(backend, H, c, x)
    ref = np.asarray(T.run_case(node(H, c, x), "oracle")[0], np.float32).reshape(got.shape)
    e_ref, e_gpu, e_cpu = T.nmse(got, ref), T.nmse(got, exact), T.nmse(ref, exact)
    plog(f"fa_mla {c}: vs oracle {e_ref:.3e}  vs twin {e_gpu:.3e}  oracle vs twin {e_cpu:.3e}")
    assert not np.isnan(got).any()
    assert e_ref <= ORACLE_F16, f"nmse {e_ref:.3e} against the oracle"
    assert e_gpu <= e_cpu * 1.01 + 1e-12, f"further from the twin ({e_gpu:.3e}) than the oracle is ({e_cpu:.3e})"


@pytest.mark.parametrize("c", [C(16, 3, 70, 1, "causal", "sep"), C(128, 1, 262, 3, "bias", "sep")], ids=["one_split", "three_splits"])
def test_aliased_and_separate_v_agree_bit_for_bit(backend, H, c):
    x = make_inputs(c)
    sep, ali = run_gpu(backend, H, c, x), run_gpu(backend, H, c._replace(vsrc="a64"), x)
    assert not np.isnan(sep).any() and np.array_equal(sep.view(np.uint32), ali.view(np.uint32))


@pytest.mark.parametrize("kw", [dict(tk=L.Q8_0), dict(kvh=2), dict(cap=50.0), dict(sinks=True), dict(bias=8.0), dict(tk=L.F32)], ids=lambda kw: next(iter(kw)) + str(next(iter(kw.values()))))
def test_supports_op_refuses(backend, H, kw):
    c = C(16, 3, 64, 1, "causal", "sep")
    assert supported(backend, H, node(H, c)), "the accepted node next to it (on a tree without the kernel nothing below says anything)"
    assert not supported(backend, H, node(H, c._replace(NH=16 * kw.get("kvh", 1)), **kw))
