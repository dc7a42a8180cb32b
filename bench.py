#!/usr/bin/env python3
"""bench.py — decode tokens/s (+ prefill tokens/s) of the MI355X backend on BASELINE.json's headline config.

Workload (N=1): BASELINE.json configs[1] — Llama-3-8B Q4_K_M (synthetic GGUF-exact tensor set, random-init: no
checkpoints exist offline), all layers on one MI355X, 2048-token prefill then batch-1 decode.  A "step" is one pass
of the hot path over one batch: llama_decode of one token (graph submit through the backend C-ABI + logits to host),
exactly what llama-box's engine loop does per iteration (llama-box/httpserver.hpp:3591, llama-bench "tg" semantics).

N>1 (one process per GPU, launched by torch.distributed.run): the same model tensor-split across ranks — column-
parallel wq/wk/wv/gate/up, row-parallel wo/down with an RCCL all-reduce of the f32 partial results over xGMI
(csrc/tp.cpp); one token stream, so "scaling" is "strong".  torch is used for plumbing only (rendezvous, barrier,
max-reduce of the timings, torch.cuda.synchronize()).

A plain run sets up, warms up, times the K steps and prints the line.  With --full the line also carries "roofline"
(dominant kernel class, hipEvent-timed on the backend's own stream in a separate eager pass of the same decode steps, then
rocprofv3 passes of their own; algorithmic bytes = the weight bytes each launch streams), "kernel_classes_us",
"cpu_baseline" (the CPU oracle = our restatement of ggml-cpu, kind "port", timed on this host's cores, rank 0, N=1) with
"parity" (the timed model's logits against it) and, for tensor-split runs, "allreduce_us" and the replica leg.

--dump-outputs DIR writes the logits of the last timed step (what llama_get_logits hands the caller) to DIR/logits.npy.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)


# kernel-class tag (graph.cpp timed_scope) -> substring of the kernel symbol rocprofv3 reports
def _class_to_symbol(cls, n_par=1, planes=False, short_rows=False):
    parts = cls.split("_")
    if cls.startswith("mmq_q8_0_skinny"):  # Q8_0 weights x 9 .. 128 columns (mmq_q80.hip); <true>: over the panel copy of the weights
        return f"k_mmq_q80_skinny<{'true' if planes else 'false'}>"
    if parts[0] == "mmq" and 2 <= n_par <= 32:
        # -np decode steps: the weight-streaming matrix-core kernel; the gate/up pair takes its tile-parallel form (mmq_skinny.hip)
        qt = {"q4": "4", "q5": "5", "q6": "6"}.get(parts[1])
        if qt is None:
            return None
        n_total = next((int(x[1:]) for x in parts if x.startswith("n") and x[1:].isdigit()), 0)
        tile_parallel = "x2" in parts and qt in ("4", "5") and n_total >= 192 * 128  # (mmq_skinny.hip skinny_tp_applies: >= 192 groups of 128 rows, no K split — the gate/up pair)
        if tile_parallel:  # Q4_K: two waves per tile (k_mmq_skinny_tp8) unless GGML_MI355X_SKINNY_TP=1; Q5_K: the four-wave form
            return "k_mmq_skinny_tp8<4>" if qt == "4" and os.environ.get("GGML_MI355X_SKINNY_TP", "2") != "1" else f"k_mmq_skinny_tp<{qt}>"
        if "+" in parts[2]:  # two formats in one launch (mmq_q4_K+q6_K_x3_..): k_mmq_skinny<4, 6, ..>
            other = {"K+q4": "4", "K+q5": "5", "K+q6": "6"}.get(parts[2])
            return f"k_mmq_skinny<{qt}, {other}, " if other else None
        return f"k_mmq_skinny<{qt}, {qt}, "
    if parts[0] != "mmvq":
        return None
    ty = {"q4": "T_Q4K", "q5": "T_Q5K", "q6": "T_Q6K", "q8": "T_Q80"}.get(parts[1])
    if ty is None:
        return None
    glu = "true" if "glu" in parts else "false"
    pro = "2" if cls.endswith("normpro") else "1"
    # (planes: the launch streamed the decode copy of its weights — the plane-layout instantiation, csrc/mmvq_types.h; Q8_0 has none; rows that are not whole groups of
    # 8 super-blocks (Qwen2-7B) run the short-group kernels T_Q*KS)
    return f"k_mmvq_stream<mi355x::{ty}{('S' if short_rows else 'P') if planes and ty != 'T_Q80' else ''}, {glu}, {pro}>"


def pmc_traffic(symbol, args):
    """HBM bytes per launch of `symbol` from rocprofv3's FETCH_SIZE (its own --pmc pass over a short decode run of this
    same script).  FETCH_SIZE is in KiB and, on gfx950, tallies the 128-byte requests of wide streaming reads at 64 B
    (MI355X_MICROARCH.md, HBM section): bytes = FETCH_SIZE * 1024 * 2."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", BENCH_PMC_CHILD="1")
    cmd = ["rocprofv3", "--kernel-trace", "--pmc", "FETCH_SIZE", "-d", out, "-o", "pmc", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--steps", "8", "--warmup", "2", "--prefill", "256" if args.np == 1 else "64", "--timing-steps", "0", "--no-cpu-baseline",
           "--pmc-traffic", "0", "--preset", args.preset, "--weight-set", args.weight_set, "--ctkv", args.ctkv, "--fa", str(args.fa), "--np", str(args.np), "--draft", str(args.draft)]
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240, check=False)
        files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            return None, "no counter_collection.csv"
        tot, n = 0.0, 0
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                if symbol in row.get("Kernel_Name", "") and row.get("Counter_Name") == "FETCH_SIZE":
                    tot += float(row["Counter_Value"])
                    n += 1
        if n == 0:
            return None, f"kernel {symbol} not in the PMC pass"
        return tot / n * 1024.0 * 2.0, f"rocprofv3 --pmc FETCH_SIZE, own pass, {n} launches, KiB x 1024 x 2 (gfx950 half-count correction)"
    except Exception as e:  # never let the optional pass break the bench line
        return None, str(e)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def rocprof_kernel_us(symbol, args):
    """Average duration of `symbol` as rocprofv3 --kernel-trace reports it (End - Start of the dispatch), over a short graph-replayed decode run of this same
    script: the number profiles/*kernel_stats.csv holds, and the one roofline.frac is computed from (the in-process per-launch events of the
    eager timing pass read ~5 % shorter)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, 0, "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="bench_kt_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", BENCH_PMC_CHILD="1")
    cmd = ["rocprofv3", "--kernel-trace", "-d", out, "-o", "kt", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--steps", "24", "--warmup", "4", "--prefill", "256" if args.np == 1 else "64", "--timing-steps", "0", "--no-cpu-baseline",
           "--pmc-traffic", "0", "--preset", args.preset, "--weight-set", args.weight_set, "--ctkv", args.ctkv, "--fa", str(args.fa), "--np", str(args.np), "--draft", str(args.draft)]
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240, check=False)
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return None, 0, "no kernel_trace.csv"
        tot, n = 0.0, 0
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                if symbol in row.get("Kernel_Name", ""):
                    tot += float(row["End_Timestamp"]) - float(row["Start_Timestamp"])
                    n += 1
        if n == 0:
            return None, 0, f"kernel {symbol} not in the trace"
        return tot / n / 1e3, n, f"rocprofv3 --kernel-trace, own pass (hipGraph replay of the same decode step), {n} launches"
    except Exception as e:  # never let the optional pass break the bench line
        return None, 0, str(e)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def dump_logits(ctx, out_dir, name, max_bytes=64 << 20):
    """The logits the last llama_decode of `ctx` handed its caller (llama_get_logits: one float32 row of the vocabulary per output) as
    out_dir/<name>.npy.  Past `max_bytes`, a fixed, seeded sample of the rows in their original order."""
    import numpy as np
    H = ctx.H
    n_out = int(H.llm_n_outputs(ctx.c))
    lg = np.ctypeslib.as_array(H.llm_get_logits(ctx.c), shape=(n_out, ctx.model.n_vocab_local))
    keep = max(1, max_bytes // lg[0].nbytes)
    if n_out > keep:
        lg = lg[np.sort(np.random.default_rng(0).choice(n_out, keep, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(lg, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--preset", default="llama3-8b-q4_k_m")
    ap.add_argument("--prefill", type=int, default=2048)
    ap.add_argument("--fa", type=int, default=1)
    ap.add_argument("--np", type=int, default=1, help="parallel sequences decoded per step (llama-box -np continuous batching)")
    ap.add_argument("--draft", type=int, default=0, help="speculative decoding: every step is one llama_decode over np x (1 + draft) tokens with logits at every position, then the "
                                                          "drafts are dropped from the cache (worst case of the verification; llama-box httpserver.hpp:4042-4069, :4696-4768)")
    ap.add_argument("--emulate-tp", type=int, default=0, dest="emulate_tp", help="ONE GPU: build and time rank 0's shard of an N-way tensor split WITHOUT any collective (the row-parallel "
                                                                                   "sums are simply not taken): the per-rank compute time of a --tensor-split run, for the time budget of DESIGN.md §6; not a throughput")
    ap.add_argument("--ubatch", type=int, default=512)
    ap.add_argument("--n-batch", type=int, default=2048, dest="n_batch", help="prompt tokens per llama_decode call (llama-box -b); several slots' prompts share a call")
    ap.add_argument("--ctkv", default="f16", choices=["f16", "q8_0", "q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl", "bf16", "f32"], help="KV cache type (llama-box --cache-type-k / --cache-type-v); the headline metric is quoted on f16")
    ap.add_argument("--layers", type=int, default=0, help="debug only: override n_layer (result is then NOT a valid bench)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--in-process", type=int, default=1, dest="in_process", help="--gpus N > 1: ALSO time the same decode with ONE process driving the N devices (-sm row through "
                                                                                   "\"ggml_backend_split_buffer_type\": what llama-box, a single process, reaches) on rank 0 while the other ranks idle")
    ap.add_argument("--replica-leg", type=int, default=1, help="tensor-split runs: also time the GPUs as independent replicas (informational field)")
    ap.add_argument("--weight-set", default="damped", choices=["damped", "chaotic"], dest="weight_set",
                    help="synthetic weight VALUES (shapes, formats and bytes are the same; kernel time does not depend on them): damped = residual branches at gain 0.08/sqrt(2 n_layer) + output rows "
                         "tied to the embeddings — the set north_star's parity bar (1e-3 on the logits, ids exact) is testable on, so the `parity` object of the line is the bar as written; "
                         "chaotic = rounds 1-5's independent random blocks (the oracle sits NMSE 8.7e-4 from itself there)")
    ap.add_argument("--cpu-steps", type=int, default=32)
    ap.add_argument("--timing-steps", type=int, default=16)
    ap.add_argument("--pmc-traffic", type=int, default=1, help="1: re-run a short decode under rocprofv3 --pmc FETCH_SIZE (own pass) for roofline.traffic")
    ap.add_argument("--full", action="store_true", help="also run what the headline does not need: the per-kernel timing pass and the rocprofv3 passes of `roofline`, the CPU "
                                                        "baseline and the parity check against it, the replica leg of tensor-split runs (--timing-steps, --pmc-traffic, "
                                                        "--no-cpu-baseline, --cpu-steps and --replica-leg act inside it)")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", help="write the logits of the last timed step to DIR/logits.npy (float32, one row per output of "
                                                                              "the step; DIR/logits_rank<r>.npy per rank with --gpus N > 1; a fixed, seeded sample of the rows "
                                                                              "beyond 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: start the N ranks ourselves, exactly as the driver's multi-GPU line does (one process
        # per GPU under torch.distributed.run, rendezvous on 127.0.0.1), and hand its exit code on.  A plain invocation used to run
        # ONE rank silently and print "n_gpus": 1.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd, env=env))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        # the ranks that came up are not the GPUs that were asked for: no line at all is better than a line about another job
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to run (launch with --nproc-per-node {args.gpus}, or plain `python bench.py --gpus {args.gpus}`)", file=sys.stderr)
        sys.exit(2)

    import numpy as np
    import torch  # first: one HIP runtime per process (torch's and /opt/rocm's share the SONAME)

    n_dev = torch.cuda.device_count()
    if n_dev < 1 or (world > n_dev and os.environ.get("BENCH_ALLOW_SHARED_GPU") != "1"):
        # one rank per GPU or nothing (BENCH_ALLOW_SHARED_GPU=1: the dry run of the multi-rank path on a one-GPU box, tests/test_gpu_model.py)
        # (every rank says so: the launcher tears the others down as soon as the first one exits, and that one need not be rank 0)
        print(f"bench.py[rank {rank}]: {world} rank(s) but {n_dev} GPU(s) visible: refusing to run", file=sys.stderr, flush=True)
        sys.exit(3)
    shared_gpu = world > n_dev
    local_rank %= n_dev
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        # one node: RCCL's bootstrap (and gloo) may use the loopback interface — the container's hostname / outward interface need
        # not resolve on the GPU box
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch.distributed as dist  # control plane on gloo; the data-path collective is RCCL inside the backend
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)

    import llama_box_amd as L
    from model_util import Context, Model, preset

    H = L.host()
    be = L.Backend(local_rank)
    hp = preset(args.preset + ("-damped" if args.weight_set == "damped" else ""))
    if args.layers > 0:
        hp.n_layer = args.layers
    parallelism = "single"
    tp_size, tp_rank = 1, 0
    if world > 1:
        # every step of the set-up is agreed on by all ranks over gloo, so that a rank that cannot load RCCL (or cannot create
        # the communicator) never leaves the others blocked in a collective: any failure -> every rank runs a full replica
        def agree(flag):
            t = torch.tensor([1 if flag else 0], dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return int(t[0]) == 1

        # (1) the one-shot peer-to-peer all-reduce (csrc/tp_p2p.hip): IPC-mapped mailboxes, the handles go round over gloo.  Serves the
        # latency-bound sums of decode; needs no RCCL and works with several ranks on one GPU (the dry run)
        err, handle = "", None
        try:
            if os.environ.get("BENCH_TP_P2P", "1") != "0":
                handle = be.tp_p2p_export(rank, world)
        except Exception as e:
            err = f"p2p export: {e}"
        handles = [None] * world
        dist.all_gather_object(handles, handle)
        p2p_ok = all(h is not None for h in handles)
        if p2p_ok:
            try:
                be.tp_p2p_attach(handles)
            except Exception as e:
                p2p_ok, err = False, f"p2p attach: {e}"
        p2p_ok = agree(p2p_ok)
        # (2) RCCL for the long messages of prompt batches (one communicator over xGMI); impossible when ranks share a GPU
        uid = [None]
        if rank == 0 and not shared_gpu and os.environ.get("BENCH_TP_RCCL", "1") != "0":
            try:
                uid[0] = be.tp_unique_id()
            except Exception as e:
                err = f"unique id: {e}"
        dist.broadcast_object_list(uid, src=0)
        rccl_ok = uid[0] is not None
        if rccl_ok:
            try:
                be.tp_init(rank, world, uid[0])
            except Exception as e:
                rccl_ok, err = False, f"comm init: {e}"
        rccl_ok = agree(rccl_ok)
        def group_check(tag):
            """Every rank sums a known vector through the backend's own collective (the path graph_compute takes) and compares: a group that
            cannot add is switched off here, before any number depends on it."""
            ok = True
            try:
                for n in (4096, 8192 * 8 + 256):  # one launch of the one-shot kernel / past its message limit (RCCL or chunks)
                    x = torch.full((n,), float(rank + 1), dtype=torch.float32, device=f"cuda:{local_rank}")
                    x[::7] += 0.5 * rank
                    dist.barrier()
                    be.tp_all_reduce(x.data_ptr(), n)
                    be.synchronize()
                    want = torch.full((n,), world * (world + 1) / 2.0, dtype=torch.float32)
                    want[::7] += 0.5 * world * (world - 1) / 2.0
                    ok = ok and bool(torch.equal(x.cpu(), want)) and int(be.stat("p2p_timeouts")) == 0
            except Exception as e:
                ok = False
                print(f"bench.py: rank {rank}: {tag} group check raised {e}", file=sys.stderr)
            return agree(ok)

        if p2p_ok and not group_check("peer-to-peer"):
            # (the mailboxes are there but do not add up on this node: leave them alone; RCCL alone carries the sums if it is there)
            be.set_option("tp_p2p", 0)
            p2p_ok = False
            err = "the peer-to-peer all-reduce failed its self-check"
        if p2p_ok or rccl_ok:
            tp_size, tp_rank = world, rank
            how = "one-shot P2P all-reduce over IPC-mapped mailboxes" + (" + RCCL for messages > 256 KiB" if rccl_ok else " (no RCCL communicator)") if p2p_ok else "RCCL all-reduce"
            parallelism = f"tp{world} (row/column tensor-split, {how}, x{2 * hp.n_layer}/token)"
        else:
            parallelism = f"replicas x{world} (tensor-split set-up failed on some rank{': ' + err if err else ''})"
    emulated = world == 1 and args.emulate_tp > 1
    if emulated:
        tp_size, tp_rank = args.emulate_tp, 0
        parallelism = f"rank 0's shard of a tp{tp_size} split ALONE on one GPU, no collectives (per-rank compute time only)"
    t_load = time.time()
    model = Model(hp, 0x5EED, be.buft, tp_rank=tp_rank, tp_size=tp_size, rowpar_buft=be.rowpar_buft() if tp_size > 1 else None)
    t_load = time.time() - t_load
    kvt = {"f16": 0, "q8_0": L.Q8_0, "q4_0": L.Q4_0, "q4_1": L.Q4_1, "q5_0": L.Q5_0, "q5_1": L.Q5_1, "iq4_nl": L.IQ4_NL, "bf16": L.BF16, "f32": -1}[args.ctkv]
    extra_leg = (args.warmup + args.steps) if (world > 1 or os.environ.get("BENCH_FORCE_TWO_LEGS") == "1") else 0  # tensor-split runs time the decode steps twice (eager, then graph replay)
    n_ctx = (args.np * (args.prefill + args.warmup + args.steps + extra_leg + args.timing_steps + 64 + args.draft) + 255) // 256 * 256
    ctx = Context(model, backend=be, n_ctx=n_ctx, n_ubatch=args.ubatch, flash_attn=args.fa, graph_reuse=1, type_k=kvt, type_v=kvt)
    rng = np.random.default_rng(1 + 0 * rank)
    T1 = 1 + args.draft  # tokens per sequence and step
    toks = rng.integers(0, hp.n_vocab, args.np * T1 * (args.prefill + args.warmup + args.steps + extra_leg + args.timing_steps + 8))

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if dist is not None:
        dist.barrier()  # every rank has its model: the first cross-rank sum is not met by a rank that is still uploading weights
    # ---- prefill (reported beside the headline; v1 path = column chunks of the bandwidth kernel)
    pos = 0
    prefill_tok_s = None
    prefill_host_split = [0, 0, 0, 0]
    if args.prefill > 0:
        # an untimed pass over the weights first: the first kernels that touch a freshly uploaded model pay for page-table population and clock ramp-up (measured on
        # one box: the first 2048-token prefill of the process 127 ms instead of 18, the 70B's first 512 tokens 1.06 s instead of 0.1) — not what a server's prompts see
        nw_ = min(64, args.prefill)
        rc, _ = ctx.decode(toks[:nw_], range(nw_), seq=[0] * nw_, want=[0] * (nw_ - 1) + [1])
        assert rc == 0, f"warm-up prefill failed rc={rc}"
        ctx.clear()
        sync()
        t0 = time.perf_counter()
        # llama-box never mixes prefill and decode in one batch (httpserver.hpp:3742, :4042), but it does fill a batch with the prompt
        # tokens of several slots up to n_batch (2048): prompts go in whole, as many per llama_decode as fit
        per_call = max(1, args.n_batch // args.prefill)
        for s0 in range(0, args.np, per_call):
            sqs = range(s0, min(args.np, s0 + per_call))
            tk, ps, sq_ids, wt = [], [], [], []
            for sq in sqs:
                tk.extend(toks[sq * args.prefill: (sq + 1) * args.prefill])
                ps.extend(range(args.prefill))
                sq_ids.extend([sq] * args.prefill)
                wt.extend([0] * (args.prefill - 1) + [1])
            rc, _ = ctx.decode(tk, ps, seq=sq_ids, want=wt)
            assert rc == 0, f"prefill failed rc={rc}"
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        prefill_tok_s = args.np * args.prefill / (t1 - t0)
        prefill_host_split = ctx.timings()  # of the last sequence's prefill: summed over its micro-batches
        pos = args.prefill

    seq_ids = list(range(args.np))

    def step(i):
        if args.draft:
            return steps(1, pos + i)
        rc, lg = ctx.decode([int(toks[(pos + i) * args.np + sq]) for sq in range(args.np)], [pos + i] * args.np, seq=seq_ids, copy_logits=False)
        assert rc == 0, f"decode failed rc={rc}"
        return lg

    def steps(n, at=None):  # n consecutive llama_decode calls issued by the host library itself (llama-box's loop is C++, not Python)
        p0 = pos if at is None else at
        rows = [[int(toks[(p0 + i) * args.np * T1 + k]) for k in range(args.np * T1)] for i in range(n)]
        rc = ctx.verify_steps(rows, args.np, args.draft, p0) if args.draft else ctx.decode_steps(rows, args.np, p0)
        assert rc == 0, f"decode failed rc={rc}"

    host_graph = {}

    def leg():  # W untimed warm-up steps, then exactly K timed steps between barrier + synchronize; max over ranks
        nonlocal pos
        if args.warmup:  # (the host library refuses a call of zero steps)
            steps(args.warmup)
        pos += args.warmup
        g0 = be.stat("graph_launches")
        gl0 = be.stat("graph_launch_host_ns")
        host0 = {k: be.stat(k) for k in ("graph_key_host_ns", "graph_compute_host_ns", "graph_key_fast_hits", "graph_captures", "graph_early_captures", "graph_exec_updates", "eager_graphs", "graph_shadow_captures", "graph_capture_walk_ns", "graph_exec_update_ns", "graph_shadow_eager_ns")}
        sync()
        t0 = time.perf_counter()
        steps(args.steps)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t1 = time.perf_counter()
        pos += args.steps
        el = t1 - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t[0])
        gs = be.stat("graph_launches") - g0
        # host time inside graph_compute per timed step (the GPU idles while the host recognises the graph it is about to replay: VERDICT r04 #6)
        host_graph.update({"graph_key_us": round((be.stat("graph_key_host_ns") - host0["graph_key_host_ns"]) / 1e3 / max(1, gs), 2),
                           "graph_compute_us": round((be.stat("graph_compute_host_ns") - host0["graph_compute_host_ns"]) / 1e3 / max(1, args.steps), 2),
                           "replays_recognised_in_place": int(be.stat("graph_key_fast_hits") - host0["graph_key_fast_hits"]),
                           # steps that were NOT replays (a -np engine outgrows its 256-cell cache view every few steps): captured at first sighting / of those,
                           # patched into the previous executable graph / run eagerly
                           "captures": int(be.stat("graph_captures") - host0["graph_captures"]), "captures_at_first_sighting": int(be.stat("graph_early_captures") - host0["graph_early_captures"]),
                           "executable_graph_updates": int(be.stat("graph_exec_updates") - host0["graph_exec_updates"]), "eager_steps": int(be.stat("eager_graphs") - host0["eager_graphs"]),
                           # round 6: a capture at first sighting runs behind the step's own eager launches; host time per capture of the walk into the capture, of
                           # hipGraphExecUpdate / instantiate, and of the eager walk in front of it
                           "captures_in_the_shadow_of_the_step": int(be.stat("graph_shadow_captures") - host0["graph_shadow_captures"]),
                           "capture_walk_us": round((be.stat("graph_capture_walk_ns") - host0["graph_capture_walk_ns"]) / 1e3 / max(1, be.stat("graph_captures") - host0["graph_captures"]), 1),
                           "exec_update_us": round((be.stat("graph_exec_update_ns") - host0["graph_exec_update_ns"]) / 1e3 / max(1, be.stat("graph_captures") - host0["graph_captures"]), 1),
                           "shadow_eager_walk_us": round((be.stat("graph_shadow_eager_ns") - host0["graph_shadow_eager_ns"]) / 1e3 / max(1, be.stat("graph_shadow_captures") - host0["graph_shadow_captures"]), 1)})
        return el, gs, (be.stat("graph_launch_host_ns") - gl0) / 1e3 / max(1, gs)

    def headline(el, extra_note=""):  # the contract's fields for a K-step time (everything else is added to it below)
        st = 1 if tp_size > 1 or world == 1 else world
        draft_note = f" with {args.draft} drafts per sequence (speculative-decoding batch shape, M = {args.np * T1})" if args.draft else ""
        return {
            "metric": "decode tokens/sec (batch-1) + prefill tok/s, Llama-3-8B Q4_K_M" if args.preset == "llama3-8b-q4_k_m" and args.np == 1 and args.draft == 0 and not emulated else
                      f"decode tokens/sec ({'batch-1' if args.np == 1 else f'-np {args.np} aggregate'}" + (f", {T1} positions per sequence and step verified: 1 sampled + {args.draft} drafts, all rejected" if args.draft else "")
                      + f") + prefill tok/s, {args.preset} [secondary configuration, not the headline metric]" + (" [ONE RANK'S SHARE OF A TENSOR SPLIT, NO COLLECTIVES: a time budget input, not a throughput]" if emulated else ""),
            "value": round(st * args.np * T1 * args.steps / el, 2), "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(el / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "strong" if tp_size > 1 else "weak", "vs_baseline": None,
            "dtype": ("q8_0 weights x q8_0 activations" if "q8_0" in args.preset else ("q5_K/q6_K" if "q5_k" in args.preset else "q4_K/q6_K") + " weights x q8_K activations") + " (int8 dot, f32 accumulate)",
            "data": "synthetic (GGUF-exact tensor set, directly sampled quant blocks, random token ids; weight values: " + ("damped + peaked set — residual branches at gain 0.08/sqrt(2 n_layer), output rows tied to the embeddings" if args.weight_set == "damped" else "independent random blocks") + ")",
            "config": {"workload": f"{args.preset}: {args.prefill}-token prefill then {'batch-1' if args.np == 1 else f'-np {args.np} continuous-batching'} decode{draft_note}, flash_attn={args.fa}, kv_cache={args.ctkv}, n_ctx={n_ctx}, n_ubatch={args.ubatch}" + (f" [DEBUG n_layer={args.layers}]" if args.layers else ""),
                       "parallelism": parallelism + extra_note + (" [DRY RUN: the ranks share one GPU]" if shared_gpu else "")},
        }

    tp_legs = None
    two_legs = (tp_size > 1 and not emulated) or os.environ.get("BENCH_FORCE_TWO_LEGS") == "1"  # (the variable: exercise this branch on one GPU)
    if two_legs:
        # Tensor split: the K steps are timed twice — eager launches first (the form that needs nothing of RCCL but stream order), then the
        # same steps captured and replayed as hipGraphs with the all-reduces inside (never yet run on multi-GPU hardware).  The faster leg
        # is `value`; if the graph leg does not come back, a watchdog prints the eager line and ends the process instead of hanging the job.
        import threading
        be.set_option("graphs", 0)
        el_eager, _, _ = leg()
        if tp_size > 1:
            tmo = torch.tensor([int(be.stat("p2p_timeouts"))], dtype=torch.int64)
            dist.all_reduce(tmo, op=dist.ReduceOp.MAX)
            if int(tmo[0]) > 0:
                # the one-shot all-reduce timed out somewhere (never seen on the boxes of the build; its spins are bounded so that this can be
                # reported instead of hanging): its sums are garbage -> with a communicator, switch it off everywhere and time the leg again
                if rccl_ok:
                    be.set_option("tp_p2p", 0)
                    parallelism += " [peer-to-peer all-reduce timed out: RCCL only]"
                    el_eager, _, _ = leg()
                else:
                    if rank == 0:
                        print("bench.py: the peer-to-peer all-reduce timed out and there is no RCCL communicator to fall back to", file=sys.stderr)
                    sys.exit(4)
        deadline = max(60.0, 30.0 * el_eager * (1.0 + args.warmup / max(1, args.steps)))

        def give_up():
            if rank == 0:
                out = headline(el_eager, " [graph-replay leg timed out: eager launches]")
                out["prefill_tok_s"] = round(prefill_tok_s, 1) if prefill_tok_s else None
                print(json.dumps(out), flush=True)
            os._exit(0)

        dog = threading.Timer(deadline, give_up)
        dog.daemon = True
        dog.start()
        be.set_option("graphs", 1)
        try:
            el_graph, graph_steps, graph_launch_host_us = leg()
        except AssertionError as e:  # a failed replay: keep the eager number
            el_graph, graph_steps, graph_launch_host_us = float("inf"), 0, 0.0
            parallelism += f" [graph-replay leg failed: {e}]"
        dog.cancel()
        tp_legs = {"eager_ms_per_step": round(el_eager / args.steps * 1e3, 4), "graph_replay_ms_per_step": round(el_graph / args.steps * 1e3, 4) if el_graph != float("inf") else None}
        elapsed = min(el_eager, el_graph)
    else:
        elapsed, graph_steps, graph_launch_host_us = leg()
    streams = 1 if tp_size > 1 or world == 1 else world
    tok_s = streams * args.np * args.steps / elapsed  # (sequence-steps per second: what the byte accounting below multiplies by)
    host_split = [x / max(1, args.steps) for x in ctx.timings()]
    if args.dump_outputs:  # before anything else decodes on this context: its logits are still the last timed step's
        dump_logits(ctx, args.dump_outputs, "logits" if world == 1 else f"logits_rank{rank}")

    # ---- per-kernel-class timing pass (eager, hipEvents on the backend's stream) and the rocprofv3 passes of the roofline: --full only
    roofline = None
    classes = {}
    if args.full:
        try:
            be.set_option("timing", 1)
            for i in range(args.timing_steps):
                step(i)
            classes = be.timing_report()
            be.set_option("timing", 0)
            pos += args.timing_steps
            classes.pop("_bracket_noop", None)
            mm = {k: v for k, v in classes.items() if k.startswith("mmvq") or k.startswith("mmq")}
            if mm:
                dom = max(mm, key=lambda k: mm[k][1])
                cnt, ms, nbytes = mm[dom]
                # the streaming mat-vec launches carry their own start/stop events (hipExtLaunchKernelGGL: the dispatch packet's
                # begin/end timestamps, what rocprofv3 reads too), so this is the kernel's duration, not a host-side bracket
                avg_us = ms * 1e3 / cnt
                ach = nbytes / cnt / (avg_us * 1e-6) / 1e9
                roofline = {"bound": "hbm", "kernel": dom, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                            "traffic": None, "launches": cnt, "avg_us": round(avg_us, 2), "alg_bytes_per_launch": round(nbytes / cnt),
                            "timing": "per-launch start/stop hipEvents (hipExtLaunchKernelGGL) on the backend stream, eager pass of the same decode steps"}
        except Exception as e:
            roofline = {"error": str(e)}
        if roofline and "kernel" in roofline and args.pmc_traffic and rank == 0 and world == 1 and not os.environ.get("BENCH_PMC_CHILD"):
            sym = _class_to_symbol(roofline["kernel"], args.np, planes=int(be.stat("decode_copy_launches")) > 0, short_rows=(hp.n_embd % 2048) != 0)
            if sym:
                torch.cuda.synchronize()
                tr, how = pmc_traffic(sym, args)
                roofline["traffic"] = round(tr) if tr else None
                roofline["traffic_source"] = how
                # `frac` from the duration rocprofv3 reports for the kernel (what profiles/ holds); the in-process per-launch events beside it
                us, n_l, how_t = rocprof_kernel_us(sym, args)
                roofline["frac_hipevent"], roofline["avg_us_hipevent"] = roofline["frac"], roofline["avg_us"]
                if us:
                    ach_r = roofline["alg_bytes_per_launch"] / (us * 1e-6) / 1e9
                    roofline.update({"achieved": round(ach_r, 1), "frac": round(ach_r / HBM_PEAK_GBS, 4), "frac_rocprof": round(ach_r / HBM_PEAK_GBS, 4), "avg_us": round(us, 2), "avg_us_rocprof": round(us, 2),
                                     "timing": how_t + "; *_hipevent: per-launch start/stop hipEvents (hipExtLaunchKernelGGL) on the backend stream, eager pass of the same decode steps"})
                else:
                    roofline["frac_rocprof"] = None
                    roofline["timing"] += f" [rocprofv3 pass unavailable: {how_t}]"

    # ---- tensor-split runs: the same decode with ONE process driving the N devices — llama-box is a single process (engine.cpp:87-95): -sm row -ts 1,1,...
    # reaches "ggml_backend_split_buffer_type", whose graphs the backend runs as tensor parallelism over its own devices (csrc/tp_inproc.cpp: sharded
    # attention + KV cache, the same one-shot all-reduce between the devices, no launcher).  Rank 0 does it on a fresh backend instance while the other
    # ranks wait at a barrier; a watchdog turns a step that does not come back into an "error" field, never into a hung job.
    in_process = None
    if world > 1 and args.in_process and tp_size > 1 and not emulated and args.np == 1 and args.draft == 0:
        if rank == 0:
            import ctypes as C
            import threading
            try:
                n_logical = int(H.ggml_backend_reg_dev_count(be.reg))
                if n_logical < world:
                    raise RuntimeError(f"{n_logical} device(s) visible to rank 0, {world} needed")
                be_ip = L.Backend(local_rank)
                split_fn = be_ip.proc("ggml_backend_split_buffer_type", C.c_void_p, [C.c_int, C.POINTER(C.c_float)])
                arr = (C.c_float * 16)(*([1.0] * world + [0.0] * (16 - world)))
                buft = split_fn(local_rank, arr)
                done = threading.Event()
                box = {}

                def leg_ip():
                    try:
                        m_ip = Model(hp, 0x5EED, be_ip.buft, split_buft=buft)
                        n_ctx_ip = (args.prefill + extra_leg + args.warmup + args.steps + 64 + 255) // 256 * 256
                        c_ip = Context(m_ip, backend=be_ip, n_ctx=n_ctx_ip, n_ubatch=args.ubatch, flash_attn=1, graph_reuse=1)
                        p_ip = 0
                        if args.prefill > 0:
                            rc_, _ = c_ip.decode(toks[:args.prefill], range(args.prefill), want=[0] * (args.prefill - 1) + [1])
                            assert rc_ == 0, f"prefill rc={rc_}"
                            p_ip = args.prefill
                        if extra_leg:  # the same cache depth as the one-process-per-GPU leg it is compared with (that one ran its eager leg first): ADVICE r05
                            assert c_ip.decode_steps([[int(toks[p_ip + i])] for i in range(extra_leg)], 1, p_ip) == 0
                            p_ip += extra_leg
                        if args.warmup:
                            assert c_ip.decode_steps([[int(toks[p_ip + i])] for i in range(args.warmup)], 1, p_ip) == 0
                        p_ip += args.warmup
                        g0_, a0_ = be_ip.stat("graph_launches"), be_ip.stat("allreduces")
                        be_ip.synchronize()
                        t0_ = time.perf_counter()
                        assert c_ip.decode_steps([[int(toks[p_ip + i])] for i in range(args.steps)], 1, p_ip) == 0
                        be_ip.synchronize()
                        el_ = time.perf_counter() - t0_
                        box.update({"value": round(args.steps / el_, 2), "unit": "tokens/s", "ms_per_step": round(el_ / args.steps * 1e3, 4), "graph_replayed_steps": int(be_ip.stat("graph_launches") - g0_),
                                    "allreduces_per_step": (be_ip.stat("allreduces") - a0_) / args.steps, "devices": int(be_ip.stat("ip_devices")),
                                    "graphs_as_tensor_parallel": int(be_ip.stat("ip_graphs")), "graphs_declined": int(be_ip.stat("ip_declined")), "p2p_timeouts": int(be_ip.stat("p2p_timeouts")),
                                    "input_copies": int(be_ip.stat("ip_input_copies")), "output_copies": int(be_ip.stat("ip_output_copies")),
                                    "note": "ONE process (rank 0) drives all devices through \"ggml_backend_split_buffer_type\" (-sm row -ts 1,...): csrc/tp_inproc.cpp; flash attention on"})
                        c_ip.free(); m_ip.free()
                    except Exception as e:  # noqa: BLE001
                        box["error"] = str(e)
                    finally:
                        done.set()

                th = threading.Thread(target=leg_ip, daemon=True)
                th.start()
                if not done.wait(timeout=max(120.0, 200.0 * elapsed)):
                    box = {"error": "the in-process leg did not come back (watchdog)"}
                in_process = dict(box)
                if done.is_set():
                    be_ip.close()
            except Exception as e:  # noqa: BLE001
                in_process = {"error": str(e)}
        if dist is not None:
            dist.barrier()

    # ---- tensor-split runs: the same GPUs as independent replicas (one full model and one sequence each), beside the headline value.
    # Batch-1 decode of a model that fits one GPU is all-reduce-latency-bound under tensor split (Multi-GPU); what N GPUs
    # are worth as N data-parallel engines is the other half of the picture.  Informational: `value` stays the tensor-split number.
    w_bytes = model.stream_bytes()
    replicas = None
    if args.full and ((tp_size > 1 and not emulated and args.replica_leg) or (world > 1 and args.replica_leg == 2)):  # (2: exercise the leg in the single-GPU dry run)
        try:
            ctx.free(); model.free()
            ctx = model = None
            model_r = Model(hp, 0x5EED, be.buft)
            ctx_r = Context(model_r, backend=be, n_ctx=n_ctx, n_ubatch=args.ubatch, flash_attn=args.fa, graph_reuse=1, type_k=kvt, type_v=kvt)
            if args.prefill > 0:
                rc, _ = ctx_r.decode(toks[:args.prefill], range(args.prefill), want=[0] * (args.prefill - 1) + [1])
                assert rc == 0
            rows_w = [[int(toks[args.prefill + i])] for i in range(args.warmup)]
            if rows_w:
                assert ctx_r.decode_steps(rows_w, 1, args.prefill) == 0
            rows_t = [[int(toks[args.prefill + args.warmup + i])] for i in range(args.steps)]
            sync()
            tr0 = time.perf_counter()
            assert ctx_r.decode_steps(rows_t, 1, args.prefill + args.warmup) == 0
            torch.cuda.synchronize()
            dist.barrier()
            el = torch.tensor([time.perf_counter() - tr0], dtype=torch.float64)
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
            ctx_r.free(); model_r.free()
            replicas = {"value": round(world * args.steps / float(el[0]), 2), "unit": "tokens/s", "scaling": "weak",
                        "note": f"{world} independent batch-1 decodes, one full model per GPU, same barrier / max-over-ranks timing"}
        except Exception as e:
            replicas = {"error": str(e)}

    # ---- CPU baseline: the oracle (restated ggml-cpu), same model shape, on this host's cores
    cpu_baseline = None
    parity = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            import ctypes as C
            import shutil
            import harness as T
            t_c = time.time()
            lib = T.oracle()
            lib.oracle_set_fast.restype = C.c_int
            fast = int(lib.oracle_set_fast(1))  # AVX2 restatement of ggml-cpu's x86 block dots (oracle/ggml_cpu_ref.c): timing leg only
            mc = Model(hp, 0x5EED, H.ggml_backend_cpu_buffer_type())
            nmax = lib.oracle_max_threads()
            # what the host offers THIS container: the cgroup's CFS quota (16 CPUs on the GPU boxes of round 5, whose host shows 256 logical CPUs).  A team
            # beyond it is descheduled by the kernel for most of its wall time — round 4's probe over {all, half, 96, 64, 32} never looked below 32 and
            # reported 13 tok/s where 8 threads deliver twice that (profiles/r05_cpu_scaling.txt)
            quota = T.cpu_quota()
            nmax = max(1, min(nmax, quota))
            # thread count: the best of a short probe around the quota
            best = (0.0, nmax)
            for nth in sorted({nmax, max(1, nmax - 1), max(1, nmax - 2), max(1, nmax - 4), max(1, nmax * 3 // 4), max(1, nmax // 2)}, reverse=True):
                cc = Context(mc, compute=T.oracle_compute_fn(nth), n_ctx=256, flash_attn=args.fa, n_threads=nth, type_k=kvt, type_v=kvt)
                cc.decode([int(toks[0])], [0])  # touch the weights / wake the pool
                tp0 = time.perf_counter()
                for i in range(3):
                    cc.decode([int(toks[1 + i])], [1 + i])
                rate = 3 / (time.perf_counter() - tp0)
                cc.free()
                if rate > best[0]:
                    best = (rate, nth)
            nth = best[1]
            cc = Context(mc, compute=T.oracle_compute_fn(nth), n_ctx=256, flash_attn=args.fa, n_threads=nth, type_k=kvt, type_v=kvt)
            cpu_rows = [cc.decode([int(toks[0])], [0])[1][0]]
            for i in range(4):  # warm
                cpu_rows.append(cc.decode([int(toks[1 + i])], [1 + i])[1][0])
            tc0 = time.perf_counter()
            for i in range(args.cpu_steps):
                cpu_rows.append(cc.decode([int(toks[5 + i])], [5 + i], copy_logits=True)[1][0])
            tc = time.perf_counter() - tc0
            lib.oracle_set_fast(0)
            found = [b for b in ("llama-box", "llama-bench", "llama-cli") if shutil.which(b)]
            cpu_baseline = {"value": round(args.cpu_steps / tc, 3), "unit": "tokens/s", "cores": nth, "kind": "port", "cpu_quota_of_this_container": quota, "host_logical_cpus": os.cpu_count(),
                            "effective_GBps": round(mc.stream_bytes() * args.cpu_steps / tc / 1e9, 1),  # weight bytes one token streams x tokens/s: what the host's DRAM delivered
                            "numa_nodes": len([d for d in os.listdir("/sys/devices/system/node") if d.startswith("node") and d[4:].isdigit()]) if os.path.isdir("/sys/devices/system/node") else 1,
                            "sample": f"{args.cpu_steps} warm batch-1 decode steps at n_past 5..{4 + args.cpu_steps} of the same synthetic {args.preset} model; CPU restatement of ggml-cpu (oracle/): "
                                      + ("AVX2 block dots as ggml-cpu's x86 kernels compute them (same integers, FMA lane accumulation)" if fast else "generic scalar block dots (no AVX2 build)")
                                      + f", OpenMP pool of {nth} threads (best of a probe over thread counts up to the container's CPU quota, {quota} of the host's {os.cpu_count()} logical CPUs), weight pages interleaved over the NUMA nodes / first-touched by many threads (ggml_lite.cpp spread_pages); NOT llama-box's binary"
                                      + (f" — binaries found on this host: {found}" if found else " (no llama-box / llama-bench / llama-cli on this host)"),
                            "setup_s": round(time.time() - t_c - tc, 1)}
            cc.free()
            # ---- parity of the timed model at full depth: the tokens the CPU leg just decoded (positions 0 .. 4 + cpu_steps, one
            # llama_decode each) go through a FRESH context of the GPU backend; logits row by row against the CPU leg's.  The yardstick beside it: the
            # oracle against itself — its generic scalar block dots against the x86 lane order the timed leg ran (same integers, another f32 order).
            if model is not None and tp_size == 1:
                try:
                    cpu_rows = np.stack(cpu_rows)
                    n_par_rows = len(cpu_rows)
                    cgp = Context(model, backend=be, n_ctx=256, flash_attn=args.fa, graph_reuse=1, type_k=kvt, type_v=kvt)
                    gpu_rows = np.stack([cgp.decode([int(toks[i])], [i])[1][0] for i in range(n_par_rows)])
                    cgp.free()
                    n_gen = min(n_par_rows, int(os.environ.get("BENCH_PARITY_GENERIC_STEPS", "16")))
                    cgn = Context(mc, compute=T.oracle_compute_fn(nmax), n_ctx=256, flash_attn=args.fa, n_threads=nmax, type_k=kvt, type_v=kvt)
                    gen_rows = np.stack([cgn.decode([int(toks[i])], [i])[1][0] for i in range(n_gen)])
                    cgn.free()
                    top2 = np.sort(cpu_rows, axis=1)
                    margin = top2[:, -1] - top2[:, -2]
                    agree = np.argmax(gpu_rows, axis=1) == np.argmax(cpu_rows, axis=1)
                    d_oo = float(np.max(np.abs(gen_rows - cpu_rows[:n_gen])))
                    decisive = margin > 2.0 * d_oo
                    span = float(cpu_rows.max() - cpu_rows.min())
                    parity = {"nmse": float(T.nmse(gpu_rows, cpu_rows)), "max_abs": float(np.max(np.abs(gpu_rows - cpu_rows))),
                              "max_abs_rel_to_logit_range": float(np.max(np.abs(gpu_rows - cpu_rows))) / span, "logit_range": span, "bar": "north_star: logits within 1e-3 (of the logit range), greedy ids exact",
                              "within_bar": bool(float(np.max(np.abs(gpu_rows - cpu_rows))) <= 1e-3 * span and bool(np.all(agree[decisive]))), "weight_set": args.weight_set,
                              "argmax_agree": f"{int(agree.sum())}/{len(agree)}",
                              "argmax_agree_where_margin_exceeds_2x_oracle_vs_oracle": f"{int((agree & decisive).sum())}/{int(decisive.sum())}",
                              "oracle_vs_oracle_nmse": float(T.nmse(gen_rows, cpu_rows[:n_gen])), "oracle_vs_oracle_max_abs": d_oo,
                              "rows": n_par_rows, "oracle_vs_oracle_rows": n_gen,
                              "what": f"{args.preset}, all {hp.n_layer} layers: {n_par_rows} batch-1 llama_decode calls at n_past 0..{n_par_rows - 1} on a fresh GPU context vs the CPU leg's logits (oracle, x86 lane order); "
                                      f"oracle-vs-oracle = the generic scalar oracle vs that leg on the first {n_gen} rows (same integer block sums, another f32 summation order)"}
                except Exception as e:
                    parity = {"error": str(e)}
            mc.free()
            mc = None
            if model is not None and tp_size == 1 and (args.np > 1 or args.draft):
                # a continuous batch: the batch-1 rows above went through the mat-vec kernels; this line's own kernels (the 2..32-column forms, position-list attention) are checked by
                # tests/test_gpu_full_depth.py's procedure on fresh models of the same preset: the prompts of np sequences in one llama_decode (logits at every position), then
                # teacher-forced steps of np tokens, against the oracle in ggml-cpu's x86 lane order (the generic scalar order is the second opinion on the prompt rows)
                try:
                    from test_gpu_full_depth import full_depth_parity
                    plines = []
                    pb = full_depth_parity(be, H, plines.append, args.preset + ("-damped" if args.weight_set == "damped" else ""), args.fa, n_prompt=2, n_dec=2, n_par=args.np, ref_fast=True,
                                           n_var_dec=0, kv=(kvt, kvt), check=False)
                    span_b = pb["max_abs"] / max(pb["max_abs_rel_to_logit_range"], 1e-30)
                    pb["within_bar"] = bool(pb["max_abs_rel_to_logit_range"] <= 1e-3 and pb["argmax_agree_at_decisive_positions"].split("/")[0] == pb["argmax_agree_at_decisive_positions"].split("/")[1])
                    pb["logit_range"] = span_b
                    pb["weight_set"] = args.weight_set
                    parity = {"batch_1_rows": parity, "continuous_batch": pb}
                except Exception as e:
                    parity = {"batch_1_rows": parity, "continuous_batch": {"error": str(e)}}
        except Exception as e:
            cpu_baseline = {"error": str(e)}

    # prefill against the matrix-core roofline: 2 flop per weight of the layer mat-muls per token (the output matrix runs for the
    # last token only) + causal attention (QK^T and PV: 2 x 2 x n_embd x mean visible positions per token and layer)
    prefill_roofline = None
    if prefill_tok_s and tp_size == 1:
        E, FF, KV = hp.n_embd, hp.n_ff, hp.n_head_kv * hp.n_embd_head
        w_layer = E * E + 2 * E * KV + E * E + 3 * E * FF
        flop_tok = 2.0 * hp.n_layer * w_layer + hp.n_layer * 4.0 * E * (args.prefill / 2.0)
        ach = flop_tok * (prefill_tok_s / args.np) * args.np / 1e12
        prefill_roofline = {"bound": "mfma", "achieved": round(ach, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(ach / 2500.0, 4),
                            "flop_per_token": round(flop_tok), "note": "dense f16 MFMA peak; the GEMMs run on the int8 matrix cores (2x rate) with two digit passes per weight"}
    if rank == 0:
        kv_per_tok = int(2 * hp.n_layer * (hp.n_head_kv // tp_size) * hp.n_embd_head * {"f16": 2, "bf16": 2, "f32": 4, "q8_0": 34 / 32, "q4_0": 18 / 32, "iq4_nl": 18 / 32, "q4_1": 20 / 32, "q5_0": 22 / 32, "q5_1": 24 / 32}[args.ctkv])
        n_past = args.prefill + extra_leg + args.warmup + args.steps // 2  # (tensor-split runs: the leg `value` comes from is the second one)
        job_bytes = (w_bytes + args.np * kv_per_tok * n_past) * (tok_s / streams / args.np)
        note_ip = ""
        if in_process and in_process.get("value") and in_process.get("devices") == world and in_process.get("graphs_declined") == 0:
            mp_value = args.steps / elapsed
            if in_process["value"] > mp_value:  # the faster of the two forms is the line's value; both are whole-job numbers of the same decode
                note_ip = f" [value = ONE process driving the {world} devices (-sm row, what llama-box reaches): {in_process['value']} tok/s; one process per GPU: {mp_value:.2f} tok/s]"
                elapsed = args.steps / in_process["value"]
                tok_s = args.steps / elapsed
            else:
                note_ip = f" [one process per GPU; ONE process driving the {world} devices (-sm row, what llama-box reaches): {in_process['value']} tok/s]"
        out = headline(elapsed, note_ip)
        out["config"].update({"n_past_mid": n_past, "weight_bytes_per_token_per_gpu": w_bytes, "kv_bytes_per_token_per_gpu": kv_per_tok * n_past})
        out.update({
            "tensor_split_legs": tp_legs,
            "prefill_tok_s": round(prefill_tok_s, 1) if prefill_tok_s else None,
            "prefill_host_us": {"build": round(prefill_host_split[0], 1), "inputs": round(prefill_host_split[1], 1), "compute+sync": round(prefill_host_split[2], 1), "logits_d2h": round(prefill_host_split[3], 1)} if prefill_tok_s else None,
            "prefill_roofline": prefill_roofline,
            "decode_hbm_frac_of_8TBs": round(job_bytes / 8e12, 4),
            "in_process_tensor_split": in_process, "replicas_on_the_same_gpus": replicas,
            # device time of one row-parallel sum (hipEvents on the backend's stream around k_p2p_all_reduce / the RCCL call, eager timing pass): fills DESIGN §6's budget row on real xGMI
            "allreduce_us": round(classes["tp_all_reduce"][1] * 1e3 / max(1, classes["tp_all_reduce"][0]), 2) if "tp_all_reduce" in classes else None,
            "tp_stats": {"allreduces": int(be.stat("allreduces")), "p2p_launches_issued": int(be.stat("p2p_allreduces")), "p2p_timeouts": int(be.stat("p2p_timeouts"))} if tp_size > 1 and not emulated else None,
            # the decode copy (round 6): K-quant matrices kept a second time in the plane layout the batch-1 mat-vec kernels stream with non-temporal loads (csrc/repack.hip)
            "decode_copy": {"tensors": int(be.stat("decode_copy_tensors")), "bytes": int(be.stat("decode_copy_bytes")), "launches_streaming_it": int(be.stat("decode_copy_launches")),
                            "step_heads_in_one_launch": int(be.stat("step_heads"))},
            "graph_replayed_steps": int(graph_steps), "hipGraphLaunch_host_us": round(graph_launch_host_us, 1), "graph_compute_host_us_per_step": host_graph,
            "host_us_per_step": {"build": round(host_split[0], 1), "inputs": round(host_split[1], 1), "compute+sync": round(host_split[2], 1), "logits_d2h": round(host_split[3], 1)},
            "roofline": roofline, "cpu_baseline": cpu_baseline, "parity": parity,
            "kernel_classes_us": {k: round(v[1] * 1e3 / max(1, v[0]), 2) for k, v in sorted(classes.items())},
            "model_load_s": round(t_load, 1),
        })
        print(json.dumps(out))
    if ctx is not None:
        ctx.free()
        model.free()
    be.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
