#!/usr/bin/env python3
"""Headline benchmark: whole-node TEPS of multi-source BFS on RMAT-26 (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
             --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W)

Config (BASELINE.json config 3): RMAT scale 26 (n = 2^26, m = 16 n = 2^30 undirected edges,
Graph500 A/B/C/D = .57/.19/.19/.05, scrambled ids), 1024 random query groups of 16 sources,
round-robin across the ranks (main.cu:304-307). Every rank generates the identical graph in its
own HBM (deterministic counter-based generator, no broadcast) — synthetic data, as the reference
ships no dataset. One step = the reference's "Computation" phase (main.cu:301-400): BFS of every
local group + F(U) + the global min-reduction (one RCCL all-reduce). TEPS counts, per group, the
undirected edges of the components its sources reach (Graph500 convention), summed
over all 1024 groups, divided by the step time. Total work is fixed as N grows: strong scaling.

A plain run does only what the headline needs: preprocessing, one untimed edge-counting pass (the
TEPS numerator), with several ranks the selection pass over the candidate decompositions, the
warm-up and the K timed steps. --full adds the untimed extras: the cold step (cold_step_ms), the
selection pass even when there is nothing to choose, the last timed step's F checked against the
untimed pass, and --verify groups checked against the per-group distance solver.
--dump-outputs DIR writes the last timed step's results (F.npy, argmin.npy; float64) for
comparing two builds: graph and queries are seeded, so equal arguments give equal inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

METRIC = "TEPS (whole node) on RMAT-26 multi-source BFS at 1/2/4/8 MI355X"
XCHG = {"hybrid": ", all-to-all exchange", "hybrid-coded": ", coded exchange",
        "hybrid-p2p": ", point-to-point exchange overlapped with phase A"}


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int) -> int:
    """Re-run this script under torch.distributed.run with n ranks on this node (a child process:
    nothing here has initialised the GPU, and exec-ing a GPU process is not allowed). Each rank
    then supervises its worker (fallback_chain)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}",
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=dict(os.environ, OMP_NUM_THREADS=os.environ.get(
        "OMP_NUM_THREADS", "4")))


def fallback_chain(dist: str):
    """Attempts of a supervised multi-rank run, each only if the previous gave no result: the
    requested run; for auto, the same without the point-to-point exchange pieces (the candidate
    least exercised between real peers); then round robin, the reference's decomposition
    (main.cu:303-307), which uses nothing but small all-reduces; last, round robin with those
    all-reduces over gloo (host memory: no RCCL communicator at all, same kernels and timing
    boundary; the JSON's backend says so)."""
    chain = [(f"--dist {dist}", [])]
    if dist == "auto":
        chain.append(("--dist auto --no-p2p", ["--dist", "auto", "--no-p2p"]))
    if dist != "roundrobin":
        chain.append(("--dist roundrobin", ["--dist", "roundrobin"]))
    chain.append(("--dist roundrobin --backend gloo", ["--dist", "roundrobin", "--backend", "gloo"]))
    return chain


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--group-size", type=int, default=16)
    ap.add_argument("--algo", default="bitpar")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--qseed", type=int, default=7)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure (all untimed): the cold step, the "
                         "selection pass even for a single decomposition, the timed F checked "
                         "against the untimed pass, and --verify")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy "
                         "(float64): F (all groups, gathered over the ranks) and argmin "
                         "(1-based minK, minF)")
    ap.add_argument("--verify", type=int, default=8,
                    help="with --full: check this many groups (over all ranks) of the timed F "
                         "against the per-group distance solver (untimed; 0 = off)")
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--wide-degree", type=int, default=0)
    ap.add_argument("--max-words", type=int, default=0)
    ap.add_argument("--backend", default=None,
                    help="torch.distributed backend (default nccl = RCCL); gloo lets several ranks "
                         "share one GPU for testing")
    ap.add_argument("--dist", default="auto",
                    choices=["auto", "roundrobin", "hybrid", "hybrid-coded", "hybrid-p2p"],
                    help="multi-GPU decomposition: round-robin query groups (main.cu:304-307) or "
                         "hybrid (levels 1-2 vertex-partitioned, then query-partitioned; its "
                         "exchange one dense all-to-all, a zero-word coded one, or point-to-point "
                         "pieces overlapped with phase A); auto = run each feasible one (untimed, "
                         "max over ranks) and time the fastest")
    ap.add_argument("--no-p2p", action="store_true",
                    help="auto without the hybrid-p2p candidate (the supervisor's second attempt "
                         "when the first one gave no result)")
    ap.add_argument("--relabel", type=int, default=1,
                    help="renumber vertices by descending degree after generation (preprocessing)")
    ap.add_argument("--test-corrupt", default="",
                    help=argparse.SUPPRESS)  # tests only: candidate whose F is falsified
    args = ap.parse_args()
    # --gpus N without a launcher: start the N ranks ourselves (one process per GPU over RCCL),
    # before this process touches the GPU, and hand back the child's exit status
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        return launch_ranks(args.gpus)
    if world_env is not None and int(world_env) != args.gpus and \
            os.environ.get("MSBFS_FORCE_DIST") != "1":
        print(f"bench: --gpus {args.gpus} but WORLD_SIZE={world_env}", file=sys.stderr)
        return 2
    from msbfs.parallel import launch
    if launch.supervised():
        # a torchrun rank: run the measurement as a worker child, and fall back to safer
        # decompositions if it gives no result (this process never touches the GPU)
        return launch.supervise([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                fallback_chain(args.dist))
    metric = METRIC if args.scale == 26 else METRIC.replace("RMAT-26", f"RMAT-{args.scale}")

    import msbfs
    from msbfs.ops import native
    from msbfs.parallel import distributed as D
    from msbfs.parallel import hybrid as H

    world = int(os.environ.get("WORLD_SIZE", "1"))
    # (one process: no torch at all, see D.init_from_env; several ranks: torch.distributed)
    ctx = D.init_from_env(backend=args.backend, use_gpu=True)
    dev = ctx.device
    if ctx.distributed:
        import torch
        import torch.distributed as tdist

        def sync():
            torch.cuda.synchronize(dev)
        pg_size = tdist.get_world_size() if tdist.is_initialized() else 1
        cur_dev = torch.cuda.current_device()
    else:
        def sync():
            native.check(native.lib().msbfs_device_sync())
        pg_size, cur_dev = 1, dev
    # which GPU every rank drives: one per rank under RCCL (it refuses duplicates anyway)
    devices = D.allgather_int(cur_dev, ctx)
    if ctx.backend == "nccl" and ctx.world > 1 and len(set(devices)) != len(devices):
        print(f"bench: ranks share GPUs under RCCL: {devices}", file=sys.stderr)
        return 2
    t_setup = time.perf_counter()
    g = msbfs.DeviceGraph.rmat(args.scale, args.edgefactor, args.seed, device=dev)
    relabelled = False
    if args.relabel:
        try:
            g.relabel_by_degree()
            relabelled = True
        except msbfs.native.MsbfsError as e:  # e.g. RMAT-30: no room for a second col array
            print(f"bench: relabel skipped: {e}", file=sys.stderr)
    qs = msbfs.QuerySet.random(g.n, args.groups, args.group_size, args.qseed)
    solver = msbfs.Solver(g, args.algo, max_groups=qs.K, alpha=args.alpha, beta=args.beta,
                          wide_degree=args.wide_degree, max_words=args.max_words)
    # graph-derived tables, and the query-dependent ones of this rank's groups: preprocessing
    # (main.cu:235-298), so that neither the untimed first run nor a timed one builds anything
    solver.prepare(qs.subset(D.round_robin(qs.K, ctx.rank, ctx.world)))
    # Every rank must pick the same candidates (hybrid and round-robin call different
    # collectives), but hybrid_max_groups() depends on the free HBM each rank saw: agree on it.
    # (the hybrid exchange moves rows by vertex id: every rank must number vertices alike)
    hybrid_local = (ctx.distributed and args.algo == "bitpar" and ctx.world <= H.MAX_PARTS
                    and 1 <= qs.K <= solver.hybrid_max_groups())
    same_ids = D.allreduce_max(float(relabelled), ctx) == -D.allreduce_max(-float(relabelled), ctx)
    hybrid_ok = D.allreduce_max(0.0 if hybrid_local else 1.0, ctx) == 0.0 and same_ids
    if args.dist.startswith("hybrid") and not hybrid_ok:
        print("bench: hybrid mode needs >1 rank, --algo bitpar and K <= one pass", file=sys.stderr)
        return 2
    # (point-to-point pieces last: a hang there ends the attempt after everything else ran)
    auto = ["roundrobin", "hybrid", "hybrid-coded"] + ([] if args.no_p2p else ["hybrid-p2p"])
    candidates = {"auto": auto if hybrid_ok else ["roundrobin"],
                  "roundrobin": ["roundrobin"], "hybrid": ["hybrid"],
                  "hybrid-coded": ["hybrid-coded"], "hybrid-p2p": ["hybrid-p2p"]}[args.dist]
    plans, cand_err = {}, {}
    for m in candidates:
        err = ""
        try:
            if m.startswith("hybrid"):
                runner = H.HybridRunner(solver, qs.K, ctx, coded=m == "hybrid-coded",
                                        chunks=H.DEFAULT_CHUNKS if m == "hybrid-p2p" else 1)
                plans[m] = (runner, runner.idx)
            else:
                rr = D.round_robin(qs.K, ctx.rank, ctx.world)
                plans[m] = (qs.subset(rr), rr)
        except Exception as e:  # noqa: BLE001 (a candidate that cannot be set up is dropped)
            err = f"{type(e).__name__}: {e}"[:240]
        if not D.agree_ok(not err, ctx):
            cand_err[m] = err or "setup failed on another rank"
            plans.pop(m, None)
    candidates = [m for m in candidates if m in plans]
    if "roundrobin" not in plans and args.dist in ("auto", "roundrobin"):
        print(f"bench: round robin could not be set up: {cand_err}", file=sys.stderr)
        return 3
    sync()
    setup_s = time.perf_counter() - t_setup

    def step(m, checked=False):
        runner = plans[m][0]
        if m.startswith("hybrid"):
            res = runner.run(qs, checked=checked)
            F, st = res.F, res.stats
        elif checked:
            r = D.checked(lambda: solver.run(runner), ctx, "round robin")
            F, st = r.F, r.stats
        else:
            r = solver.run(runner)  # round robin: the rank's query subset
            F, st = r.F, r.stats
        if args.test_corrupt == m and len(F):  # (tests: a candidate with a wrong answer)
            F = F.copy()
            F[0] += 1
        return F, st

    rr_idx = D.round_robin(qs.K, ctx.rank, ctx.world)
    rr_qs = qs.subset(rr_idx)
    cold_ms = None
    if args.full:
        # cold step: the first computation after preprocessing (round robin, the reference's
        # decomposition, with its blocking argmin; main.cu:301-400), reported next to the warm
        # steps
        D.barrier(ctx)
        sync()
        t_cold = time.perf_counter()
        D.packed_argmin(solver.run(rr_qs).F, rr_idx, qs.K, ctx)
        sync()
        cold_ms = D.allreduce_max(time.perf_counter() - t_cold, ctx) * 1e3
    # untimed: TEPS numerator (traversed edges per group)
    r0 = solver.run(rr_qs, count_edges=True)
    total_edges = int(D.allreduce_sum_i64(np.array([int(r0.edges.sum())], np.int64), ctx)[0])
    # untimed: every candidate decomposition once (correctness check against the round-robin
    # pass via the gathered F vector, and its time, max over ranks); the fastest one is timed.
    # A plain run with a single candidate has nothing to choose and skips the pass.
    select = args.full or len(candidates) > 1
    F_ref = D.gather_F(r0.F, rr_idx, qs.K, ctx) if select or args.steps <= 0 else None
    # Each candidate runs twice and keeps its faster time: the first run of a decomposition can
    # carry one-time costs (e.g. RCCL setting up the all-to-all's peer connections) that would
    # otherwise decide the choice. Round robin goes first; a candidate that raises (on any rank)
    # or whose gathered F differs from the untimed round-robin pass is excluded (every rank
    # decides alike) and reported in candidate_errors; only round robin failing ends the run.

    def run_gathered(m):
        Fm, st = step(m, checked=True)
        return D.gather_F(Fm, plans[m][1], qs.K, ctx), st  # identical on every rank

    cand_ms = {}
    if select:
        cand_ms, errs = D.evaluate_candidates(candidates, run_gathered, F_ref, ctx,
                                              reps=2 if ctx.distributed else 1,
                                              sync=sync)
        cand_err.update(errs)
        for m, e in errs.items():
            if ctx.rank == 0:
                print(f"bench: candidate {m} excluded: {e}", file=sys.stderr)
        if "roundrobin" in cand_err or not cand_ms:
            print(f"rank {ctx.rank}: no verified decomposition: {cand_err}", file=sys.stderr)
            return 3
        mode = min(cand_ms, key=cand_ms.get)
    elif candidates:
        mode = candidates[0]
    else:
        print(f"rank {ctx.rank}: no decomposition could be set up: {cand_err}", file=sys.stderr)
        return 3
    local_idx = plans[mode][1]
    # the step's global argmin: an async 8-byte MIN all-reduce, waited for once the next step's
    # BFS has run (the last one inside the timed region)
    amin = D.AsyncArgmin(ctx)

    def run_steps(k):
        pend, res, st = None, (-1, -1), {}
        for _ in range(k):
            F, st = step(mode)
            if pend is not None:
                res = amin.wait(pend)
            pend = amin.start(F, local_idx, qs.K)
        if pend is not None:
            res = amin.wait(pend)
        return F if k else None, st, res

    run_steps(max(0, args.warmup))
    D.barrier(ctx)
    sync()
    t0 = time.perf_counter()
    F, stats, (min_k, min_f) = run_steps(args.steps)
    sync()
    D.barrier(ctx)
    dt = time.perf_counter() - t0
    dt = D.allreduce_max(dt, ctx)  # slowest rank
    ms = dt / max(1, args.steps) * 1e3
    trace = solver.level_trace()  # last timed step: per-level direction and host wall time
    # hybrid: per-phase wall ms of the last timed step, max over ranks, and the all-to-all rate
    phases = {}
    if mode.startswith("hybrid"):
        for key in ("phase_a_wall_ms", "exchange_ms", "phase_c_wall_ms", "phase_a_ms",
                    "phase_c_ms"):
            phases[key] = round(D.allreduce_max(float(stats.get(key) or 0.0), ctx), 3)
        sent = D.allreduce_max(float(stats.get("sent_bytes", 0)), ctx)
        xms = phases.get("exchange_ms") or 0.0
        phases["alltoall_GBps_per_rank"] = round(sent / (xms * 1e6), 1) if xms > 0 else None
        phases["chunks"] = int(stats.get("chunks", 1))  # exchange pieces overlapped with phase A
    # the last timed step's F of all ranks, gathered (without timed steps: the untimed pass's)
    F_last = None
    if args.steps <= 0:
        F_last = F_ref
        k = msbfs.argmin_first(F_ref)
        min_k, min_f = k, (int(F_ref[k]) if k >= 0 else -1)
    elif args.full or args.dump_outputs:
        F_last = D.gather_F(F, local_idx, qs.K, ctx)
    if args.dump_outputs and ctx.rank == 0:
        # what a caller of the timed path receives: F of every group and the argmin (1-based
        # minK as the report prints it); F < 2^53, so float64 holds it exactly
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "F.npy"), np.asarray(F_last, dtype=np.float64))
        np.save(os.path.join(args.dump_outputs, "argmin.npy"),
                np.array([int(min_k) + 1, int(min_f)], dtype=np.float64))
    # ---- --full: untimed self-check of the timed result: the last timed step's F equals the
    # untimed pass, and the first groups of every rank equal the per-group distance solver's F
    # (an independent algorithm: one int32 distance per vertex, main.cu:40-89)
    if args.full and not np.array_equal(F_last, F_ref):
        bad = np.flatnonzero(F_last != F_ref)[:8]
        print(f"rank {ctx.rank}: timed F differs from the untimed pass at groups {bad}",
              file=sys.stderr)
        return 3
    verified, verify_err = 0, ""
    if args.full and args.verify > 0:
        nv = min(len(rr_idx), -(-args.verify // ctx.world))
        ok = 1.0
        if nv:
            try:
                with msbfs.Solver(g, "dist") as ds:
                    rv = ds.run(qs.subset(rr_idx[:nv]))
                if not np.array_equal(rv.F, F_ref[rr_idx[:nv]]):
                    print(f"rank {ctx.rank}: VERIFY FAILED: bitpar {F_ref[rr_idx[:nv]]} vs dist "
                          f"{rv.F}", file=sys.stderr)
                    ok = 0.0
            except msbfs.native.MsbfsError as e:  # e.g. RMAT-30: no room for the distance array
                verify_err = str(e)[:120]
                nv = 0
        if D.allreduce_max(1.0 - ok, ctx) > 0:
            return 3
        verified = int(D.allreduce_sum_i64(np.array([nv], np.int64), ctx)[0])
    value = total_edges / (ms / 1e3) if ms > 0 else 0.0
    if ctx.rank == 0:
        out = {
            "metric": metric,
            "value": value,
            "unit": "TEPS",
            "n_gpus": ctx.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "exact-int (int32 CSR, u64 bitsets)",
            "data": "synthetic (device-generated Graph500 RMAT, random query groups)",
            "verified": verified,
            "config": {
                "model": f"rmat{args.scale}-ef{args.edgefactor}",
                "global_batch": qs.K,
                "seq_len": args.group_size,
                "parallelism": (f"hybrid{ctx.world} (levels 1-2 vertex-partitioned, then "
                                f"query-partitioned{XCHG[mode]})"
                                if mode.startswith("hybrid") else f"dp{ctx.world}"),
                "algo": args.algo,
                "n": g.n, "m": g.m,
                "traversed_edges": total_edges,
                "min_k": int(min_k) + 1, "min_f": int(min_f),
                "levels": stats.get("levels"), "td_levels": stats.get("td_levels"),
                "bu_levels": stats.get("bu_levels"), "batches": stats.get("batches"),
                "dirs": "".join(t["dir"] for t in trace),
                "level_ms": [round(t["ms"], 3) for t in trace],
                "setup_s": round(setup_s, 3), "relabel": relabelled,
                "full": args.full,
                **({"cold_step_ms": round(cold_ms, 3)} if cold_ms is not None else {}),
                "candidates_ms": {k: round(v, 3) for k, v in cand_ms.items()},
                "candidate_errors": cand_err,
                "devices": devices, "process_group_size": pg_size, "backend": ctx.backend,
                **({"phases": phases} if phases else {}),
                **({"timed_F_equals_untimed": True} if args.full else {}),
                "verified_groups_vs_dist_solver": verified,
                **({"verify_skipped": verify_err} if verify_err else {}),
            },
        }
        launch.emit_result(json.dumps(out))
    solver.close()
    g.close()
    D.shutdown(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
