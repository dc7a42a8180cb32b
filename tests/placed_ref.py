"""Results placed by hand over an operand's memory: the helper, the legality checker and the case table of tests/test_placed_ref_host.py (CPU) and
tests/test_gpu_placed.py (MI355X).

tests/harness.py gives every tensor its own block, so no op-level graph ever has a result that shares bytes with a tensor the graph read earlier — what a graph
allocator produces all the time, and what about fifty decisions in csrc/graph.cpp (the ranges_overlap guards, the address key of the quantised-activation area,
act_area_kept_for, the sum-of-squares record) exist for.  Here a node is placed the way ops_ref._as_view does it: view_src / view_offs / nb are set on the op node
before G.compute, and the context allocator then puts the node's bytes inside the chosen root tensor.  No allocator heuristic takes part: a case's layout is the
same on every run.

`legal(gf)` says whether a correct allocator could have produced the layout (the rule is in its docstring).  A case that fails it is a bug of the test.  A placement
changes where bytes live and nothing about the values: test_placed_ref_host.py pins the oracle on the placed graph to the oracle on the same graph with every
tensor in its own block, bit for bit, so the oracle on the placed graph is the GPU's reference.  (Family D's NORM and SSM_CONV are no ops of the oracle: those
cases are held to the bits of the unfused kernels and to their families' float64 twins; family E's MUL_MAT_ID and ADD_ID neither: moe_ref's composite reference.)

Every build function has the signature build(g, placed=True, control=False) and returns a Built: `placed=False` is the same graph with every tensor in its own block,
`control=True` the neighbouring graph on which the fused form under test IS taken (asserted by its statistic, so that the placed run proves something).

Listed in the issue and NOT in the table, because the placement cannot be reached legally (legal() was not bent for them):
  A1, single MUL_MAT over its own activation row: x's last reader is the MUL_MAT itself, and MUL_MAT is not an op ggml runs in place.  (The gate / up / SwiGLU form of
      A1 is legal — the GLU node is placed after x's last reader, the second mat-mul — and is in the table.)
  A4, the consumer's result over the deferred norm's MUL node: the MUL's last reader is that consumer.
  A6, wo's result over the FLASH_ATTN_EXT node it reads: the same.
ggml-alloc allocates a node before it releases the node's parents, so none of the three can come out of it; the guards in run_mul_mat_q that speak of them are
defensive.
"""
import contextlib
import ctypes as C
from collections import namedtuple

import numpy as np

import harness as T
import llama_box_amd as L
from ops_ref import _as_view  # noqa: F401  (the placement primitive; re-exported)

F32 = L.F32
OUTPUT = 2  # GGML_TENSOR_FLAG_OUTPUT
VIEW_OP_NAMES = ("NONE", "VIEW", "RESHAPE", "PERMUTE", "TRANSPOSE")
# ggml-alloc.c: ggml_op_can_inplace
INPLACE_OP_NAMES = ("SCALE", "DIAG_MASK_ZERO", "DIAG_MASK_INF", "ADD", "ADD_ID", "ADD1", "SUB", "MUL", "DIV", "SQR", "SQRT", "LOG", "UNARY", "ROPE", "ROPE_BACK", "SILU_BACK",
                    "RMS_NORM", "SET_ROWS", "SOFT_MAX", "SOFT_MAX_BACK")
_ops = {}


def op_number(name):
    if not _ops:
        H = L.host()
        for i in range(256):
            s = H.ggml_op_name(i)
            if not s or s.decode() in _ops:
                break
            _ops[s.decode()] = i
    return _ops[name]


def _addr(tp):
    return C.addressof(tp.contents) if tp else 0


# ------------------------------------------------------------------------------------------------ placement
def place(g, node, root, offs=0):
    """The f32 op node `node`, contiguous, at byte offset offs of root's block (root: a leaf or an earlier node that is no view itself)."""
    assert not root.contents.view_src and node.contents.type == F32
    ne = node.contents.ne
    assert offs + 4 * ne[0] * ne[1] * ne[2] * ne[3] <= g.H.ggml_nbytes(root), "the placed node does not fit its root"
    return _as_view(node, root, [4, 4 * ne[0], 4 * ne[0] * ne[1], 4 * ne[0] * ne[1] * ne[2]], offs)


def scale_inplace(g, a, s):
    """ggml_scale_inplace over the contiguous f32 tensor a (a root, or a node placed at offset 0 of nothing: its own block)."""
    return place(g, g.H.ggml_scale(g.ctx, a, s), a, 0)


# ------------------------------------------------------------------------------------------------ legality
def _graph_facts(H, gf):
    """(nodes, info): info maps a storage tensor's address -> dict(t, idx, root, lo, hi, last) — idx -1 for a leaf, last the index of the last node that reads it
    (views resolved to the tensor they show), -1 if none."""
    view_ops = {op_number(n) for n in VIEW_OP_NAMES}
    nodes = [gf.contents.nodes[i] for i in range(gf.contents.n_nodes)]
    idx_of = {_addr(n): i for i, n in enumerate(nodes)}

    def storage(t):  # the tensor whose bytes a view shows
        while t.contents.op in view_ops and t.contents.op != 0 and t.contents.src[0]:
            t = t.contents.src[0]
        return t

    info = {}

    def note(t):
        t = storage(t)
        a = _addr(t)
        if a not in info:
            root = t.contents.view_src if t.contents.view_src else t
            lo = t.contents.view_offs if t.contents.view_src else 0
            info[a] = dict(t=t, idx=idx_of.get(a, -1), root=_addr(root), lo=lo, hi=lo + H.ggml_nbytes(t), last=-1)
        return info[a]

    for i, n in enumerate(nodes):
        if n.contents.op in view_ops:
            continue
        note(n)
        for s in range(10):
            if n.contents.src[s]:
                f = note(n.contents.src[s])
                f["last"] = max(f["last"], i)
    return nodes, info, storage


def violations(gf):
    """Why an allocator could not have produced this graph's layout; empty when it could.

    Walks the nodes in order.  For a placed node w (an op node with view_src set) at index j, every other tensor t whose byte range overlaps w's and that exists
    before w (a leaf, or a node of a lower index) must satisfy one of
      * t's last reader is at an index < j (readers of views count as readers of the tensor they show) and t is not flagged OUTPUT;
      * t is an operand of w at the identical address and strides, w's op is one ggml runs in place (ggml_op_can_inplace), t is not flagged OUTPUT and no node
        after w reads t (w is its last reader: what ggml-alloc asks before it reuses a parent).
    A tensor of a higher index that overlaps w is judged from its own side when it is placed; the root itself must come before w."""
    H = L.host()
    nodes, info, storage = _graph_facts(H, gf)
    view_ops = {op_number(n) for n in VIEW_OP_NAMES}
    inplace = {op_number(n) for n in INPLACE_OP_NAMES}
    bad = []
    for j, w in enumerate(nodes):
        wc = w.contents
        if wc.op in view_ops or not wc.view_src:
            continue
        fw = info[_addr(w)]
        name = lambda f: f"'{f['t'].contents.name.decode()}' (node {f['idx']})"  # noqa: E731
        if wc.view_src.contents.view_src:
            bad.append(f"{name(fw)}: its root is a view itself")
        for a, ft in info.items():
            if a == _addr(w) or ft["root"] != fw["root"] or ft["hi"] <= fw["lo"] or fw["hi"] <= ft["lo"]:
                continue
            tc = ft["t"].contents
            if ft["idx"] > j:
                if not tc.view_src:
                    bad.append(f"{name(fw)} is placed in {name(ft)}, which is produced later")
                continue
            if tc.flags & OUTPUT:
                bad.append(f"{name(fw)} overwrites the graph output {name(ft)}")
                continue
            if ft["last"] < j:
                continue
            operand = False
            for s in range(10):
                sp = wc.src[s]
                if sp and _addr(storage(sp)) == a and _addr(sp) == a:
                    operand = operand or (ft["lo"] == fw["lo"] and tc.type == wc.type and all(tc.nb[d] == wc.nb[d] and tc.ne[d] == wc.ne[d] for d in range(4)))
            if operand and wc.op in inplace and ft["last"] == j:
                continue
            bad.append(f"{name(fw)} overwrites {name(ft)}, which node {ft['last']} still reads")
    return bad


def legal(gf):
    return not violations(gf)


def victim_reader(gf):
    """(j, r) for the graph's first placed node w (index j) that has one: r the index of the last node other than w that reads a tensor w overlaps.  None if no node
    is placed over a tensor that was read."""
    H = L.host()
    nodes, info, storage = _graph_facts(H, gf)
    view_ops = {op_number(n) for n in VIEW_OP_NAMES}
    for j, w in enumerate(nodes):
        if w.contents.op in view_ops or not w.contents.view_src:
            continue
        fw = info[_addr(w)]
        r = -1
        for a, ft in info.items():
            if a == _addr(w) or ft["root"] != fw["root"] or ft["hi"] <= fw["lo"] or fw["hi"] <= ft["lo"] or ft["idx"] > j:
                continue
            for k in range(j):
                u = nodes[k].contents
                if u.op not in view_ops and any(u.src[s] and _addr(storage(u.src[s])) == a for s in range(10)):
                    r = max(r, k)
        if r >= 0:
            return j, r
    return None


def move_before_reader(gf):
    """Mutates gf: the placed node of victim_reader() is moved to the position of its victim's last reader, which then runs after it.  Only placement is judged
    afterwards, so the node's own operands may now follow it."""
    j, r = victim_reader(gf)
    arr = gf.contents.nodes
    order = [_addr(arr[i]) for i in range(gf.contents.n_nodes)]  # (addresses: arr[i] is a window on the slot, not a copy of the pointer)
    order.insert(r, order.pop(j))
    for i, a in enumerate(order):
        arr[i] = C.cast(a, L.TP)
    return j, r


# ------------------------------------------------------------------------------------------------ running
Built = namedtuple("Built", "outs first probes", defaults=((), ()))  # outs: read back and flagged OUTPUT; first: expanded before them, unflagged; probes: read back, not part of the graph's outputs
# kind: 'deterministic' or 'race' (the issue's two kinds); placed_node: a node of the graph is placed (False: the guard is about order alone); oracle: the C oracle
# has every op of the graph (False: NORM, SSM_CONV — those families are judged against their float64 twins and the unfused kernels' bits, as their own tests do)
Case = namedtuple("Case", "id family build kind placed_node oracle", defaults=(True, True))
Case.__repr__ = lambda c: c.id


@contextlib.contextmanager
def graph(case, placed=True, control=False):
    """The case's graph as G.compute would build it (flags included), unallocated: for legal()."""
    g = T.G("oracle")
    try:
        b = case.build(g, placed, control)
        H = g.H
        gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
        for o in b.first:
            H.ggml_build_forward_expand(gf, o)
        for o in b.outs:
            H.ggml_set_output(o)
            H.ggml_build_forward_expand(gf, o)
        yield gf
    finally:
        g.free()


def run(case, target, placed=True, control=False, n_threads=4):
    """(outs, probes) as arrays."""
    g = T.G(target)
    try:
        b = case.build(g, placed, control)
        outs = g.compute(list(b.outs), n_threads, expand_first=list(b.first))
        return outs, [g.read(p) for p in b.probes]
    finally:
        g.free()


# ------------------------------------------------------------------------------------------------ cases
QNAME = {L.Q4_K: "q4_K", L.Q8_0: "q8_0"}
EPS = 1e-5


def _row(rng, n, rows=1):
    return (rng.standard_normal((rows, n)) * rng.uniform(0.5, 3.0, (rows, 1))).astype(np.float32)


def a1_glu(qt):
    """gate / up / SwiGLU over one row, the GLU node over x: no f32 prologue — the row is quantised by a launch of its own (kernel_launches +2; unplaced +1)."""
    rng = np.random.default_rng(1100 + qt)
    K, N = 512, 64
    wg, wu, x = T.rand_weight(qt, K, N, rng), T.rand_weight(qt, K, N, rng), _row(rng, K)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K], x, "x")
        gt = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], wg), xt)
        ut = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], wu), xt)
        s = H.ggml_swiglu_split(g.ctx, gt, ut)
        if placed and not control:
            place(g, s, xt)
        return Built([s])

    return Case(f"A1-glu-{QNAME[qt]}", "A", build, "race")


def a2(qt):
    """RMS_NORM -> MUL deferred into two mat-vec prologues, the MUL in place over x: both products from the norm of the ORIGINAL x, the MUL never written."""
    rng = np.random.default_rng(1200 + qt)
    K, NQ, NK = 512, 64, 32
    wq, wk, x, wn = T.rand_weight(qt, K, NQ, rng), T.rand_weight(qt, K, NK, rng), _row(rng, K), rng.uniform(0.5, 1.5, K).astype(np.float32)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K], x, "x")
        m = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, xt, EPS), g.new(F32, [K], wn))
        if placed and not control:
            place(g, m, xt)
        return Built([H.ggml_mul_mat(g.ctx, g.new(qt, [K, NQ], wq), m), H.ggml_mul_mat(g.ctx, g.new(qt, [K, NK], wk), m)], (), [xt])

    build.inputs = (x,)
    return Case(f"A2-{QNAME[qt]}", "A", build, "deterministic")


def a3(qt):
    """As A2 with the MUL in its own block and the FIRST consumer's result over x (x's last reader is the RMS_NORM): the pair must not be deferred — the second
    consumer's prologue would read x after the first launch wrote it."""
    rng = np.random.default_rng(1300 + qt)
    K, NQ, NK = 512, 64, 32
    wq, wk, x, wn = T.rand_weight(qt, K, NQ, rng), T.rand_weight(qt, K, NK, rng), _row(rng, K), rng.uniform(0.5, 1.5, K).astype(np.float32)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K], x, "x")
        m = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, xt, EPS), g.new(F32, [K], wn))
        q = H.ggml_mul_mat(g.ctx, g.new(qt, [K, NQ], wq), m)
        if placed and not control:
            place(g, q, xt)
        return Built([q, H.ggml_mul_mat(g.ctx, g.new(qt, [K, NK], wk), m)])

    return Case(f"A3-{QNAME[qt]}", "A", build, "deterministic")


def a5():
    """wo + residual leaves its sum of squares for the next RMS_NORM prologue (control: ss_handoffs +1); an in-place SCALE of the residual stream in between makes
    the record stale: it must be dropped, and the norm follows the scaled row.  What this pins is the hand-over's comparison of the recorded tensor with the
    RMS_NORM's source by pointer (the in-place node is another tensor at the same address); the record's invalidation by range in run_nodes is not what decides
    here — no legal layout of op nodes makes the RMS_NORM read the recorded tensor itself after another node wrote into it."""
    qt = L.Q4_K
    rng = np.random.default_rng(1500)
    K, N2 = 512, 64
    wo, w2, a, res, wn = T.rand_weight(qt, K, K, rng), T.rand_weight(qt, K, N2, rng), _row(rng, K), _row(rng, K), rng.uniform(0.5, 1.5, K).astype(np.float32)

    def build(g, placed=True, control=False):
        H = g.H
        h = H.ggml_add(g.ctx, H.ggml_mul_mat(g.ctx, g.new(qt, [K, K], wo), g.new(F32, [K], a)), g.new(F32, [K], res))
        early = H.ggml_scale(g.ctx, h, 2.0)  # (a reader of the unscaled row, in front of the in-place node)
        if not control:
            h = scale_inplace(g, h, 0.5) if placed else H.ggml_scale(g.ctx, h, 0.5)
        m = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, h, EPS), g.new(F32, [K], wn))
        return Built([early, H.ggml_mul_mat(g.ctx, g.new(qt, [K, N2], w2), m)])

    return Case("A5-q4_K", "A", build, "deterministic")


def b1():
    """MUL_MAT over X, X scaled in place, MUL_MAT over the result: same address, size and kind as the blocks in the activation area — the second product must be
    Y's."""
    qt = L.Q4_K
    rng = np.random.default_rng(2100)
    K, N, M = 256, 32, 4
    w1, w2, x = T.rand_weight(qt, K, N, rng), T.rand_weight(qt, K, N, rng), _row(rng, K, M)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K, M], x, "X")
        o1 = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w1), xt)
        y = scale_inplace(g, xt, -1.75) if placed else H.ggml_scale(g.ctx, xt, -1.75)
        return Built([o1, H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w2), y)])

    return Case("B1", "B", build, "deterministic")


def b2():
    """As B1, the writer being the absorbed tail of a fused launch: the bias ADD folded into the second mat-mul's store is placed over X (X's last reader is that
    mat-mul), and a third mat-mul reads the ADD."""
    qt = L.Q4_K
    rng = np.random.default_rng(2200)
    K, N, M = 256, 32, 4
    w1, w2, w3, x, bias = T.rand_weight(qt, K, N, rng), T.rand_weight(qt, K, K, rng), T.rand_weight(qt, K, N, rng), _row(rng, K, M), rng.standard_normal(K).astype(np.float32)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K, M], x, "X")
        o1 = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w1), xt)
        y = H.ggml_add(g.ctx, H.ggml_mul_mat(g.ctx, g.new(qt, [K, K], w2), xt), g.new(F32, [K], bias))
        if placed:
            place(g, y, xt)
        return Built([o1, H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w3), y)])

    return Case("B2", "B", build, "deterministic")


def b3():
    """RMS_NORM -> MUL read by two Q4_K mat-muls with a Q8_0 mat-mul over another input between them: the blocks in the shared activation area would not survive
    the intruder, so the producer must write the f32 rows (control, without the intruder: the quantise-only producer rms_norm_mul_quantize).  Nothing is placed."""
    rng = np.random.default_rng(2300)
    K, N, M = 256, 32, 4
    w1, w2, wi = T.rand_weight(L.Q4_K, K, N, rng), T.rand_weight(L.Q4_K, K, N, rng), T.rand_weight(L.Q8_0, K, N, rng)
    x, z, wn = _row(rng, K, M), _row(rng, K, M), rng.uniform(0.5, 1.5, K).astype(np.float32)

    def build(g, placed=True, control=False):
        H = g.H
        m = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(F32, [K, M], x), EPS), g.new(F32, [K], wn))
        o1 = H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [K, N], w1), m)
        o2 = H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [K, N], w2), m)
        if control:
            return Built([o1, o2])
        return Built([o1, H.ggml_mul_mat(g.ctx, g.new(L.Q8_0, [K, N], wi), g.new(F32, [K, M], z)), o2])

    return Case("B3", "B", build, "deterministic", False)


def sibling_m(qt):
    """Q4_K: 2 columns, the fewest batch_form sends to the int8 matrix cores (mmq_min_cols_for: 2 for Q4_K; mmq_i8_supported: M >= 2).  Q8_0: 9, where the
    weight-streaming matrix-core kernel starts."""
    return 2 if qt == L.Q4_K else 9


def _siblings(qt, seed):
    rng = np.random.default_rng(seed + qt)
    K, N, M = 512, 64, sibling_m(qt)
    ws = [T.rand_weight(qt, K, N, rng) for _ in range(3)]
    return K, N, M, ws, _row(rng, K, M), _row(rng, N, M)


def c1(qt):
    """A node between the siblings reads Z, and the third sibling's result is placed over Z: run early, at the first sibling's position, it would overwrite what
    that node has yet to read.  control: the three siblings alone."""
    K, N, M, ws, x, z = _siblings(qt, 3100)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K, M], x, "X")
        s = [H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), xt) for w in ws]
        if control:
            return Built(s)
        zt = g.new(F32, [N, M], z, "Z")
        between = H.ggml_scale(g.ctx, zt, 3.0)
        if placed:
            place(g, s[2], zt)
        return Built([s[0], between, s[1], s[2]])

    return Case(f"C1-{QNAME[qt]}", "C", build, "deterministic")


def c2(qt):
    """The third sibling's result is placed over the block of a node that is produced and read for the last time between the first sibling and the third: run
    early, the sibling's result would be overwritten by that node.  Such a node is also an operand of the node that reads it between the siblings, so
    find_mm_siblings' operand test declines the layout as well: its result test is never the only one that does."""
    K, N, M, ws, x, z = _siblings(qt, 3200)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K, M], x, "X")
        s = [H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), xt) for w in ws]
        if control:
            return Built(s)
        between = H.ggml_scale(g.ctx, g.new(F32, [N, M], z, "Z"), 3.0)
        reader = H.ggml_scale(g.ctx, between, -0.5)
        if placed:
            place(g, s[2], between)
        return Built([s[0], reader, s[1], s[2]])

    return Case(f"C2-{QNAME[qt]}", "C", build, "deterministic")


def c3(qt):
    """The third sibling carries an ADD whose addend is produced between the first sibling and the third: the ADD must not ride in the early launch's store.
    Nothing is placed: the guard is about order."""
    K, N, M, ws, x, z = _siblings(qt, 3300)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [K, M], x, "X")
        s = [H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), xt) for w in ws]
        if control:
            return Built(s)
        addend = H.ggml_scale(g.ctx, g.new(F32, [N, M], z, "Z"), 3.0)
        return Built([s[1], H.ggml_add(g.ctx, s[2], addend)], [s[0], addend], [s[0]])

    return Case(f"C3-{QNAME[qt]}", "C", build, "deterministic", False)


def _norm_chain(seed, ne0, rows):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows + 1, ne0)) * 4 + 0.5).astype(np.float32), rng.uniform(0.5, 1.5, ne0).astype(np.float32), rng.standard_normal(ne0).astype(np.float32)


def d1():
    """NORM -> MUL -> ADD, the ADD in place over x: the chain is one launch (fused_nodes +2) that reads and writes the same rows."""
    ne0, rows = 100, 3
    x, w, b = _norm_chain(4100, ne0, rows)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, [ne0, rows], x[:rows], "x")
        r = H.ggml_add(g.ctx, H.ggml_mul(g.ctx, H.ggml_norm(g.ctx, xt, EPS), g.new(F32, [ne0], w)), g.new(F32, [ne0], b))
        if placed and not control:
            place(g, r, xt)
        return Built([r])

    build.inputs = (x[:rows], w, b)
    return Case("D1", "D", build, "deterministic", True, False)


def d2():
    """As D1, x and the ADD being views of one parent, one row apart (what a recycled larger block gives): a launch that wrote the ADD's rows would overwrite
    rows of x that other workgroups have yet to read — the chain must not be absorbed past the node that overlaps."""
    ne0, rows = 100, 3
    x, w, b = _norm_chain(4200, ne0, rows)

    def build(g, placed=True, control=False):
        H = g.H
        parent = g.new(F32, [ne0, rows + 1], x, "parent")
        xt = H.ggml_view_2d(g.ctx, parent, ne0, rows, ne0 * 4, 0)
        r = H.ggml_add(g.ctx, H.ggml_mul(g.ctx, H.ggml_norm(g.ctx, xt, EPS), g.new(F32, [ne0], w)), g.new(F32, [ne0], b))
        if placed and not control:
            place(g, r, parent, ne0 * 4)
        return Built([r])

    build.inputs = (x[:rows], w, b)
    return Case("D2", "D", build, "race", True, False)


def d5():
    """SSM_CONV -> ADD(bias) -> SILU with the SILU placed over the conv input: the fused launch would write what other workgroups still read."""
    rng = np.random.default_rng(4500)
    d_conv, d_inner, n_t, n_s = 4, 70, 5, 2
    sx = (rng.standard_normal((n_s, d_inner, d_conv - 1 + n_t)) * 3).astype(np.float32)
    c, b = rng.standard_normal((d_inner, d_conv)).astype(np.float32), rng.standard_normal(d_inner).astype(np.float32)

    def build(g, placed=True, control=False):
        H = g.H
        st = g.new(F32, [d_conv - 1 + n_t, d_inner, n_s], sx, "sx")
        r = H.ggml_silu(g.ctx, H.ggml_add(g.ctx, H.ggml_ssm_conv(g.ctx, st, g.new(F32, [d_conv, d_inner], c)), g.new(F32, [d_inner], b)))
        if placed and not control:
            place(g, r, st)
        return Built([r])

    case = Case("D5", "D", build, "race", True, False)
    build.inputs = (sx, c, b)
    return case


GN_NE, GN_GROUPS, GN_EPS = (8, 8, 16, 1), 4, 1e-6  # the UNet block of tests/test_gpu_diffusion.py: the smallest shape its chains run


def _gn_inputs(seed):
    rng = np.random.default_rng(seed)
    W, Hh, Cc = GN_NE[:3]
    return (rng.standard_normal((2, Cc, Hh, W)) * 2 + 0.3).astype(np.float32), rng.uniform(0.5, 1.5, Cc).astype(np.float32), rng.standard_normal(Cc).astype(np.float32)


def d3():
    """GROUP_NORM -> MUL -> ADD -> SILU, the SILU in place over x: the whole chain is one launch (fused_nodes +3) that writes the bytes it normalises."""
    x, w, b = _gn_inputs(4300)

    def build(g, placed=True, control=False):
        H = g.H
        xt = g.new(F32, GN_NE, x[0], "x")
        r = H.ggml_add(g.ctx, H.ggml_mul(g.ctx, H.ggml_group_norm(g.ctx, xt, GN_GROUPS, GN_EPS), g.new(F32, [1, 1, GN_NE[2], 1], w)), g.new(F32, [1, 1, GN_NE[2], 1], b))
        r = H.ggml_silu(g.ctx, r)
        if placed and not control:
            place(g, r, xt)
        return Built([r])

    build.inputs = (x[:1], w, b)
    return Case("D3", "D", build, "deterministic", True, False)


def d4():
    """As D3, x and the SILU being views of one parent, one row of 8 values apart (what a recycled larger block gives): a launch that wrote the SILU's bytes would
    overwrite values of x that other workgroups have yet to read — the chain is absorbed up to the ADD (its own block) and the SILU runs on its own."""
    x, w, b = _gn_inputs(4400)
    W, Hh, Cc = GN_NE[:3]
    flat = x.reshape(-1)[: W * Hh * Cc + W]

    def build(g, placed=True, control=False):
        H = g.H
        parent = g.new(F32, [W * Hh * Cc + W], flat, "parent")
        xt = H.ggml_view_4d(g.ctx, parent, W, Hh, Cc, 1, W * 4, W * Hh * 4, W * Hh * Cc * 4, 0)
        r = H.ggml_add(g.ctx, H.ggml_mul(g.ctx, H.ggml_group_norm(g.ctx, xt, GN_GROUPS, GN_EPS), g.new(F32, [1, 1, Cc, 1], w)), g.new(F32, [1, 1, Cc, 1], b))
        r = H.ggml_silu(g.ctx, r)
        if placed and not control:
            place(g, r, parent, W * 4)
        return Built([r])

    build.inputs = (x[:1], w, b)
    return Case("D4", "D", build, "race", True, False)


def e(qt):
    """MUL_MAT_ID -> ADD_ID with the ADD_ID placed over b (b's last reader is the MUL_MAT_ID): the bias must not ride in the product's store, whose workgroups
    would write rows of b that others still read (f16 experts), or whose activation blocks were made from (Q4_K) — the ADD_ID runs as a launch of its own."""
    import moe_ref as MR

    rng = np.random.default_rng(5000 + qt)
    K, N, n_expert, n_used, n_tok = (256 if qt == L.Q4_K else 160), 33, 4, 2, 3
    W = MR.expert_weights(qt, K, N, n_expert, rng)
    b = rng.standard_normal((n_tok, n_used, K)).astype(np.float32)
    bias = rng.standard_normal((n_expert, N)).astype(np.float32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)

    def build(g, placed=True, control=False):
        H = g.H
        bt = g.new(F32, [K, n_used, n_tok], b, "b")
        sel = MR.strided_ids(g, ids, n_expert)
        r = H.ggml_add_id(g.ctx, H.ggml_mul_mat_id(g.ctx, g.new(qt, [K, N, n_expert], W), bt, sel), g.new(F32, [N, n_expert], bias), sel)
        if placed and not control:
            place(g, r, bt)
        return Built([r])

    build.inputs = (qt, W, K, N, b, bias, ids)
    return Case(f"E-{'q4_K' if qt == L.Q4_K else 'f16'}", "E", build, "race", True, False)


NF_SMALLEST = {"LIST": "layouts_dq1_g2", "MMA": "mma_t33_kv64_g1"}  # nf_ref.CASES' smallest of either form whose CONT copy is the only reader (LIST: with one
#                                                                     workgroup per (token, KV head), dq 1 — what the same-rows rule of try_fuse_attn_nf asks)


def f12(form, shifted):
    """MUL_MAT(K view, q) -> SOFT_MAX(mask) -> MUL_MAT(V^T view, p) -> CONT(PERMUTE) as nf_ref.run_probe builds it, over nf_ref's random probe.
    F1 (shifted False): the CONT's target at offset 0 of q's block, the same rows — the chain keeps the copy (fused_nodes 3: a workgroup overwrites only the q
    rows it alone has read).  F2 (shifted True): q is a view of a parent one token row longer and the target lies one row on — other rows: the copy is declined
    as the launch's target (fused_nodes 2) and runs on its own after it."""
    import nf_ref as N

    nc = next(c for c in N.CASES if c.id == NF_SMALLEST[form])
    assert nc.form == form and nc.dest == "copy" and (form == "MMA" or nc.dq == 1)
    D, NH, NKV, T_, nkv = nc.HD, nc.NH, nc.NKV, nc.T, nc.nkv
    EK = NKV * D
    memo = {}

    def probe():
        if "p" not in memo:
            p = N.random_probe(nc)
            q = np.zeros((T_ + 1, NH, D), np.float32)
            q[:T_] = p.q
            memo["p"] = (p, q, p.mask.astype(np.float32) if nc.mtype == L.F32 else p.mask)
        return memo["p"]

    def build(g, placed=True, control=False):
        H = g.H
        p, q, mask = probe()
        if shifted:
            parent = g.new(F32, [D, NH, T_ + 1], q, "q parent")
            root, qt3 = parent, H.ggml_view_3d(g.ctx, parent, D, NH, T_, D * 4, D * NH * 4, 0)
        else:
            root = qt3 = g.new(F32, [D, NH, T_], q[:T_], "q")
        qq = H.ggml_permute(g.ctx, qt3, 0, 2, 1, 3)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [EK, nkv], p.kraw), D, nkv, NKV, EK * 2, D * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [nkv, EK], p.vraw), nkv, D, NKV, nkv * 2, nkv * 2 * D, 0)
        sm = H.ggml_soft_max_ext(g.ctx, H.ggml_mul_mat(g.ctx, k, qq), g.new(nc.mtype, [nkv, p.mask.shape[0]], mask), float(nc.sc), 0.0)
        cur = H.ggml_cont_2d(g.ctx, H.ggml_permute(g.ctx, H.ggml_mul_mat(g.ctx, v, sm), 0, 2, 1, 3), D * NH, T_)
        if placed and not control:
            place(g, cur, root, D * NH * 4 if shifted else 0)
        return Built([cur])

    build.nf_case = nc
    return Case(f"F{2 if shifted else 1}-{form.lower()}", "F", build, "race" if shifted else "deterministic")


def f3():
    """One token: SOFT_MAX(K.q, mask, scale) -> MUL_MAT(V^T view, p) folded into one launch (control: fused_nodes +1), the product placed over the K.q tensor the
    soft-max reads (its last reader): workgroups would store rows of the product while others still read the logits — the fold is declined."""
    rng = np.random.default_rng(6300)
    HD, NKV, NH, nkv = 128, 2, 8, 256
    kc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((NKV * HD, nkv)).astype(np.float16)
    q = (rng.standard_normal((1, NH, HD)) * 2).astype(np.float32)
    mask = np.zeros((64, nkv), np.float32)
    mask[:, int(nkv * 0.8):] = -np.inf
    mask[:, 3] = -np.inf

    def build(g, placed=True, control=False):
        H = g.H
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], kc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [nkv, NKV * HD], vc), nkv, HD, NKV, nkv * 2, nkv * 2 * HD, 0)
        kq = H.ggml_mul_mat(g.ctx, k, H.ggml_permute(g.ctx, g.new(F32, [HD, NH, 1], q), 0, 2, 1, 3))  # [nkv, 1, NH]
        r = H.ggml_mul_mat(g.ctx, v, H.ggml_soft_max_ext(g.ctx, kq, g.new(F32, [nkv, 64], mask), 0.0883883, 0.0))  # [HD, 1, NH]
        if placed and not control:
            place(g, r, kq)
        return Built([r])

    return Case("F3", "F", build, "race")


def all_cases():
    out = []
    for qt in (L.Q4_K, L.Q8_0):
        out += [a1_glu(qt), a2(qt), a3(qt)]
    out += [a5(), b1(), b2(), b3()]
    for qt in (L.Q4_K, L.Q8_0):
        out += [c1(qt), c2(qt), c3(qt)]
    out += [d1(), d2(), d3(), d4(), d5(), e(L.F16), e(L.Q4_K)]
    out += [f12("LIST", False), f12("LIST", True), f12("MMA", False), f12("MMA", True), f3()]
    return out


CASES = {c.id: c for c in all_cases()}
