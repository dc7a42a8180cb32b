// tp.cpp — tensor parallelism, one process per GPU: RCCL all-reduce of row-parallel partial sums over xGMI.
//
// The reference has no collective at all (multi-GPU in llama.cpp is layer split or the row-split
// buffer with peer copies; no NCCL/RCCL).  `north_star` asks for --tensor-split re-implemented as sharding with an
// all-reduce of the residual, so this is new design, MI355X-first: each rank owns a column-parallel slice of
// wq/wk/wv/gate/up and a row-parallel (K-sliced) slice of wo/down; weights placed in the "RowPar" buffer type mark
// the two mat-muls per layer whose f32 partial results are summed across ranks, in-stream, right after the kernel
// (graph.cpp).  The message is n_embd x M floats (16 KiB at batch 1 for 8B, 32 KiB for 70B): latency-bound, so it
// is issued on the compute stream itself (no extra stream hop) and is capturable into the decode hipGraph.
// RCCL is dlopen()ed on first use: single-GPU runs never load the 570 MB library.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace mi355x {

struct rccl_api {
    void * handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char * (*GetErrorString)(ncclResult_t) = nullptr;
};

static rccl_api * load_rccl() {
    static rccl_api api;
    static bool tried = false;
    if (tried) return api.handle ? &api : nullptr;
    tried = true;
    const char * names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char * n : names) {
        api.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (api.handle) break;
    }
    if (!api.handle) {
        MI_ERR("cannot load RCCL: %s", dlerror());
        return nullptr;
    }
    api.GetUniqueId = (decltype(api.GetUniqueId)) dlsym(api.handle, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank)) dlsym(api.handle, "ncclCommInitRank");
    api.AllReduce = (decltype(api.AllReduce)) dlsym(api.handle, "ncclAllReduce");
    api.CommDestroy = (decltype(api.CommDestroy)) dlsym(api.handle, "ncclCommDestroy");
    api.GetErrorString = (decltype(api.GetErrorString)) dlsym(api.handle, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) {
        MI_ERR("RCCL library lacks a required symbol");
        api.handle = nullptr;
        return nullptr;
    }
    return &api;
}

struct tp_state {
    ncclComm_t comm = nullptr;  // optional since round 4: a peer-to-peer-only group has none
    int rank = 0, world = 1;
    // one-shot peer-to-peer all-reduce (tp_p2p.hip): this rank's mailbox, every rank's mailbox as mapped here, the device-side state words
    char * mbox_local = nullptr;
    char * mbox[P2P_MAX_RANKS] = {nullptr};
    unsigned * p2p_state = nullptr;
    unsigned * p2p_err_host = nullptr;  // pinned + mapped: raised by the kernel on a time-out, read by tp_check() without touching the device
    bool p2p = false;
    bool local_group = false;  // the ranks are the devices of THIS process (tp_attach_local): the peers' mailboxes are not IPC mappings
    int p2p_max_cols_bytes = 0;  // messages up to this many bytes take the one-shot path when RCCL is there too
};
static size_t mbox_bytes(int world) { return (size_t) 2 * (size_t) world * P2P_SLOT_FLOATS * 8; }

int tp_get_unique_id(void * out, size_t size) {
    rccl_api * api = load_rccl();
    if (!api || size < sizeof(ncclUniqueId)) return -1;
    ncclUniqueId id;
    if (api->GetUniqueId(&id) != ncclSuccess) return -2;
    memcpy(out, &id, sizeof(id));
    return 0;
}

int tp_init(backend_ctx * c, int rank, int world, const void * uid, size_t uid_size) {
    if (world <= 1) return 0;
    rccl_api * api = load_rccl();
    if (!api || uid_size < sizeof(ncclUniqueId)) return -1;
    ncclUniqueId id;
    memcpy(&id, uid, sizeof(id));
    tp_state * t = c->tp ? c->tp : new tp_state();  // (a peer-to-peer group may already be attached)
    t->rank = rank;
    t->world = world;
    HIP_TRY(hipSetDevice(c->device), -2);
    ncclResult_t r = api->CommInitRank(&t->comm, world, id, rank);
    if (r != ncclSuccess) {
        MI_ERR("ncclCommInitRank failed: %s", api->GetErrorString ? api->GetErrorString(r) : "?");
        if (!c->tp) delete t;
        return -2;
    }
    c->tp = t;
    // The all-reduces are enqueued on the backend's stream like every kernel, so a decode step with a communicator attached CAN be
    // captured and replayed as one hipGraph like a single-GPU step (RCCL supports stream capture; the first sighting of a topology runs
    // eagerly, which lets RCCL finish its lazy connection set-up outside a capture, and a failed capture falls back to eager execution:
    // graph.cpp).  A replay that hangs has no fallback, though, and this path has not run on multi-GPU hardware yet: with a communicator
    // attached, graphs are OPT-IN — GGML_MI355X_TP_GRAPHS=1, or the host's explicit set_option("graphs", 1) after tp_init (bench.py does
    // that for its second, watchdog-guarded leg).  ADVICE r02.
    // Only ever LOWERED here: a host that switched graphs off before tp_init keeps them off whatever the environment says.
    const char * e = getenv("GGML_MI355X_TP_GRAPHS");
    const bool env_on = e != nullptr && atoi(e) != 0;
    c->opt.graphs = c->opt.graphs && env_on;
    MI_INFO("tensor parallel rank %d / %d: hipGraph replay of steps with all-reduces is %s (GGML_MI355X_TP_GRAPHS=%s; set_option(\"graphs\", 1) after tp_init turns it on)",
            rank, world, c->opt.graphs ? "ON" : "off", e ? e : "unset");
    return 0;
}

// ---- peer-to-peer group (no RCCL needed).  Step 1, every rank: allocate the mailbox and hand out its IPC handle ...
int tp_p2p_export(backend_ctx * c, int rank, int world, void * handle_out, size_t size) {
    if (world < 2 || world > P2P_MAX_RANKS || rank < 0 || rank >= world || size < sizeof(hipIpcMemHandle_t)) return -1;
    HIP_TRY(hipSetDevice(c->device), -2);
    tp_state * t = c->tp ? c->tp : new tp_state();
    if (c->tp && (t->rank != rank || t->world != world)) { MI_ERR("tp_p2p_export: rank / world differ from the RCCL communicator's"); return -3; }
    t->rank = rank;
    t->world = world;
    if (!t->mbox_local) {
        // uncached (fine-grained) device memory: peers write it over xGMI / from another process while this rank's kernel polls it
        hipError_t e = hipExtMallocWithFlags((void **) &t->mbox_local, mbox_bytes(world), hipDeviceMallocUncached);
        if (e != hipSuccess) {
            (void) hipGetLastError();
            e = hipExtMallocWithFlags((void **) &t->mbox_local, mbox_bytes(world), hipDeviceMallocFinegrained);
        }
        if (e != hipSuccess) {
            (void) hipGetLastError();
            MI_ERR("tp_p2p_export: cannot allocate %.1f MiB of uncached mailbox memory (%s)", mbox_bytes(world) / 1048576.0, hipGetErrorString(e));
            if (!c->tp) delete t;
            return -4;
        }
        HIP_TRY(hipMemset(t->mbox_local, 0, mbox_bytes(world)), -5);  // tag 0 never matches: epochs start at 1
        HIP_TRY(hipMalloc((void **) &t->p2p_state, 64), -5);
        HIP_TRY(hipMemset(t->p2p_state, 0, 64), -5);
        HIP_TRY(hipHostMalloc((void **) &t->p2p_err_host, 64, hipHostMallocMapped | hipHostMallocPortable), -5);
        *t->p2p_err_host = 0;
        HIP_TRY(hipDeviceSynchronize(), -5);
    }
    hipIpcMemHandle_t h;
    const hipError_t e = hipIpcGetMemHandle(&h, t->mbox_local);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        MI_ERR("tp_p2p_export: hipIpcGetMemHandle failed (%s) — HSA_ENABLE_IPC_MODE_LEGACY=0 is required on this driver", hipGetErrorString(e));
        if (!c->tp) { (void) hipFree(t->mbox_local); (void) hipFree(t->p2p_state); (void) hipHostFree(t->p2p_err_host); delete t; }
        return -6;
    }
    memcpy(handle_out, &h, sizeof(h));
    c->tp = t;
    return 0;
}
// ... step 2, every rank, after the handles went round (the caller's control plane: gloo in bench.py / the tests): map the peers' mailboxes
int tp_p2p_attach(backend_ctx * c, const void * handles, size_t size) {
    tp_state * t = c->tp;
    if (!t || !t->mbox_local || size < (size_t) t->world * sizeof(hipIpcMemHandle_t)) return -1;
    HIP_TRY(hipSetDevice(c->device), -2);
    for (int r = 0; r < t->world; ++r) {
        if (r == t->rank) { t->mbox[r] = t->mbox_local; continue; }
        hipIpcMemHandle_t h;
        memcpy(&h, (const char *) handles + (size_t) r * sizeof(h), sizeof(h));
        void * p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void) hipGetLastError();
            MI_ERR("tp_p2p_attach: hipIpcOpenMemHandle of rank %d's mailbox failed (%s)", r, hipGetErrorString(e));
            return -3;
        }
        t->mbox[r] = (char *) p;
    }
    t->p2p = true;
    const char * e = getenv("GGML_MI355X_P2P_MAX_BYTES");
    t->p2p_max_cols_bytes = e ? atoi(e) : 8 * 8192 * 4;  // up to eight columns of a 70B residual stream; longer messages prefer RCCL's ring when there is one
    // as with a communicator: replayed graphs containing cross-rank waits are opt-in (a replay that hangs has no fallback; the kernel's spins are bounded)
    const bool env_on = env_flag("GGML_MI355X_TP_GRAPHS", false);
    if (!t->comm) c->opt.graphs = c->opt.graphs && env_on;
    MI_INFO("tensor parallel rank %d / %d: one-shot peer-to-peer all-reduce attached (mailbox %.1f MiB per rank%s)", t->rank, t->world, mbox_bytes(t->world) / 1048576.0,
            t->comm ? ", RCCL for longer messages" : ", no RCCL communicator");
    return 0;
}
// ---- the same group inside ONE process (tp_inproc.cpp: llama-box drives all devices from one process, engine.cpp:87-95): every device's worker
// context becomes a rank; the mailboxes are plain device allocations reached over peer access — no IPC handles, no control plane
int tp_attach_local(backend_ctx * const * ctxs, int n) {
    if (n < 2 || n > P2P_MAX_RANKS) return -1;
    for (int r = 0; r < n; ++r)
        if (ctxs[r]->tp) return -2;  // (already a rank of something else)
    std::vector<tp_state *> ts((size_t) n, nullptr);
    auto undo = [&]() {
        for (int r = 0; r < n; ++r) {
            if (!ts[(size_t) r]) continue;
            (void) hipSetDevice(ctxs[r]->device);
            if (ts[(size_t) r]->mbox_local) (void) hipFree(ts[(size_t) r]->mbox_local);
            if (ts[(size_t) r]->p2p_state) (void) hipFree(ts[(size_t) r]->p2p_state);
            if (ts[(size_t) r]->p2p_err_host) (void) hipHostFree(ts[(size_t) r]->p2p_err_host);
            delete ts[(size_t) r];
        }
        (void) hipGetLastError();
    };
    for (int r = 0; r < n; ++r) {
        tp_state * t = ts[(size_t) r] = new tp_state();
        t->rank = r;
        t->world = n;
        if (hipSetDevice(ctxs[r]->device) != hipSuccess) { undo(); return -3; }
        for (int q = 0; q < n; ++q) {  // every other device of the group may write this one's mailbox
            if (ctxs[q]->device == ctxs[r]->device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, ctxs[r]->device, ctxs[q]->device) != hipSuccess || !can) { (void) hipGetLastError(); MI_ERR("tp_attach_local: device %d cannot reach device %d", ctxs[r]->device, ctxs[q]->device); undo(); return -4; }
            if (hipDeviceEnablePeerAccess(ctxs[q]->device, 0) != hipSuccess) (void) hipGetLastError();  // (already enabled is fine)
        }
        hipError_t e = hipExtMallocWithFlags((void **) &t->mbox_local, mbox_bytes(n), hipDeviceMallocUncached);
        if (e != hipSuccess) {
            (void) hipGetLastError();
            e = hipExtMallocWithFlags((void **) &t->mbox_local, mbox_bytes(n), hipDeviceMallocFinegrained);
        }
        if (e != hipSuccess || hipMemset(t->mbox_local, 0, mbox_bytes(n)) != hipSuccess || hipMalloc((void **) &t->p2p_state, 64) != hipSuccess || hipMemset(t->p2p_state, 0, 64) != hipSuccess ||
            hipHostMalloc((void **) &t->p2p_err_host, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void) hipGetLastError();
            MI_ERR("tp_attach_local: mailbox of device %d failed", ctxs[r]->device);
            undo();
            return -5;
        }
        *t->p2p_err_host = 0;
    }
    const char * e = getenv("GGML_MI355X_P2P_MAX_BYTES");
    for (int r = 0; r < n; ++r) {
        tp_state * t = ts[(size_t) r];
        for (int q = 0; q < n; ++q) t->mbox[q] = ts[(size_t) q]->mbox_local;
        t->p2p = true;
        t->local_group = true;
        t->p2p_max_cols_bytes = e ? atoi(e) : 8 * 8192 * 4;
        ctxs[r]->tp = t;
    }
    return 0;
}

// set_option("tp_p2p", 0 / 1): stop / resume serving sums through the mailboxes (a launcher that saw time-outs falls back to RCCL).
// Switching them OFF is refused in a group that has no RCCL communicator: nothing else could carry the sums, and a row-parallel mat-mul
// without its reduction is a silently wrong model.
bool tp_p2p_enable(backend_ctx * c, bool on) {
    if (!(c->tp && c->tp->mbox_local && c->tp->mbox[c->tp->rank])) return !on;  // (no mailboxes attached: "off" is what it is)
    if (!on && c->tp->comm == nullptr) {
        MI_ERR("set_option(tp_p2p, 0) refused: this tensor-parallel group has no RCCL communicator, the mailboxes are its only transport");
        return false;
    }
    c->tp->p2p = on;
    if (!on && c->tp->p2p_err_host) *c->tp->p2p_err_host = 0;  // (the sums are RCCL's from here on: a time-out of the mailboxes is history)
    return true;
}
// set_option("tp_p2p_reset", 1), on EVERY rank of the group with all of them idle (the host's control plane: a barrier before and after):
// forgets a time-out — device word, host word, the mailboxes' tags and the epoch — so that the group can be used again
bool tp_p2p_reset(backend_ctx * c) {
    tp_state * t = c->tp;
    if (!t || !t->mbox_local || !t->p2p_state) return false;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { (void) hipGetLastError(); return false; }
    if (hipMemset(t->mbox_local, 0, mbox_bytes(t->world)) != hipSuccess || hipMemset(t->p2p_state, 0, 64) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void) hipGetLastError(); return false; }
    if (t->p2p_err_host) *t->p2p_err_host = 0;
    t->p2p = t->mbox[t->rank] != nullptr;
    return true;
}
// graph_compute's entry check: a time-out of the one-shot all-reduce means the sums of the graph(s) before were wrong, and the group's ranks may
// disagree about it.  Every graph_compute of this rank fails from then on until the HOST — which has a control plane over the ranks — either resets
// the group (set_option("tp_p2p_reset", 1) on every rank) or, with a RCCL communicator attached, switches the mailboxes off on every rank
// (set_option("tp_p2p", 0): bench.py does that after agreeing over gloo).  Never a silent wrong sum, never a rank-local change of transport.
bool tp_check(backend_ctx * c) {
    tp_state * t = c->tp;
    if (!t || !t->p2p_err_host || *(volatile unsigned *) t->p2p_err_host == 0) return true;
    MI_ERR("tensor parallel rank %d / %d: the peer-to-peer all-reduce timed out — results since then are invalid; graph_compute fails until the host resets the group "
           "(set_option tp_p2p_reset) %s", t->rank, t->world, t->comm ? "or switches it to RCCL on every rank (set_option tp_p2p 0)" : "(no RCCL communicator is attached)");
    return false;
}
int64_t tp_p2p_timeouts(backend_ctx * c) {
    if (!c->tp || !c->tp->p2p_state) return 0;
    unsigned st[3] = {0, 0, 0};
    if (hipMemcpy(st, c->tp->p2p_state, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) { (void) hipGetLastError(); return -1; }
    return (int64_t) st[2];
}

// membership, not transport: a rank of a group ALWAYS treats its row-parallel weights as partial sums — if no transport is left, the sum fails
// loudly instead of being skipped
bool tp_active(const backend_ctx * c) { return c->tp != nullptr && c->tp->world > 1; }

bool tp_all_reduce(backend_ctx * c, float * ptr, size_t n) {
    if (!tp_active(c)) return true;
    tp_state * t = c->tp;
    if (t->comm == nullptr && !t->p2p) {
        MI_ERR("tensor parallel rank %d / %d: a row-parallel sum is due and no transport is available (no RCCL communicator, mailboxes off)", t->rank, t->world);
        return false;
    }
    if (t->p2p && (t->comm == nullptr || n * sizeof(float) <= (size_t) t->p2p_max_cols_bytes)) {
        // one launch per mailbox-full (decode: ONE launch; a prompt batch without RCCL goes through in chunks)
        static const unsigned max_spins = getenv("GGML_MI355X_P2P_MAX_SPINS") ? (unsigned) atoll(getenv("GGML_MI355X_P2P_MAX_SPINS")) : 2000000u;  // seconds of polling before the group is declared broken (ranks enter their first all-reduce after a barrier of the launcher)
        for (size_t o = 0; o < n; o += P2P_SLOT_FLOATS) {
            p2p_args a{};
            a.data = ptr + o;
            a.n = (int) std::min<size_t>(P2P_SLOT_FLOATS, n - o);
            a.rank = t->rank;
            a.world = t->world;
            for (int r = 0; r < t->world; ++r) a.mbox[r] = t->mbox[r];
            a.state = t->p2p_state;
            a.err_host = t->p2p_err_host;
            a.max_spins = max_spins;
            launch_p2p_all_reduce(c->stream, a);
            c->st.kernel_launches++;
            c->st.p2p_allreduces++;
        }
        return hipGetLastError() == hipSuccess;
    }
    rccl_api * api = load_rccl();
    ncclResult_t r = api->AllReduce(ptr, ptr, n, ncclFloat32, ncclSum, c->tp->comm, c->stream);
    if (r != ncclSuccess) {
        MI_ERR("ncclAllReduce failed: %s", api->GetErrorString ? api->GetErrorString(r) : "?");
        return false;
    }
    return true;
}

bool tp_all_reduce_fused(backend_ctx * c, float * ptr, size_t n, const float * add, float * out, double * ss_out, int * ss_n) {
    if (!tp_active(c)) return false;
    tp_state * t = c->tp;
    if (!t->p2p || n > P2P_SLOT_FLOATS || (t->comm != nullptr && n * sizeof(float) > (size_t) t->p2p_max_cols_bytes)) return false;
    static const unsigned max_spins = getenv("GGML_MI355X_P2P_MAX_SPINS") ? (unsigned) atoll(getenv("GGML_MI355X_P2P_MAX_SPINS")) : 2000000u;
    p2p_args a{};
    a.data = ptr;
    a.n = (int) n;
    a.rank = t->rank;
    a.world = t->world;
    for (int r = 0; r < t->world; ++r) a.mbox[r] = t->mbox[r];
    a.state = t->p2p_state;
    a.err_host = t->p2p_err_host;
    a.max_spins = max_spins;
    a.add = add;
    a.out = out;
    a.ss_out = ss_out;
    if (ss_n) *ss_n = p2p_all_reduce_blocks(a.n);
    launch_p2p_all_reduce(c->stream, a);
    c->st.kernel_launches++;
    c->st.p2p_allreduces++;
    return hipGetLastError() == hipSuccess;
}

void tp_free(backend_ctx * c) {
    if (!c->tp) return;
    rccl_api * api = c->tp->comm ? load_rccl() : nullptr;
    if (api && c->tp->comm) api->CommDestroy(c->tp->comm);
    for (int r = 0; r < c->tp->world && r < P2P_MAX_RANKS && !c->tp->local_group; ++r)
        if (c->tp->mbox[r] && c->tp->mbox[r] != c->tp->mbox_local && hipIpcCloseMemHandle(c->tp->mbox[r]) != hipSuccess) (void) hipGetLastError();
    if (c->tp->mbox_local && hipFree(c->tp->mbox_local) != hipSuccess) (void) hipGetLastError();
    if (c->tp->p2p_state && hipFree(c->tp->p2p_state) != hipSuccess) (void) hipGetLastError();
    if (c->tp->p2p_err_host && hipHostFree(c->tp->p2p_err_host) != hipSuccess) (void) hipGetLastError();
    delete c->tp;
    c->tp = nullptr;
}

}  // namespace mi355x
