"""python -m msbfs -g <graph.bin> -q <query.bin> -gn <numGPU> [options]

The torch.distributed twin of the native CLI (`_bin/msbfs`, launched with mpirun): launch with
`torchrun --nproc-per-node N -m msbfs ...` for one rank per GPU over RCCL (or gloo on CPU).
Same flags and the same 7-line report as the reference (main.cu:203-224, 403-414); unknown
tokens are ignored; fewer than 4 arguments print the usage line and exit 255.
"""
import sys


def main(argv=None) -> int:
    argv = list(sys.argv if argv is None else argv)
    from .parallel import distributed as D
    if len(argv) < 5:
        import os
        if int(os.environ.get("RANK", "0")) == 0:
            print(f"Usage: mpirun -np <ranks> {argv[0]} -g <graph.bin> -q <query.bin> -gn <numGPU>",
                  file=sys.stderr)
        return 255
    from .engine import Engine, JobConfig
    cfg = JobConfig()
    json_out = False
    dist_out = None  # --dist-out FILE: the winning group's distance row (n x int32 LE)
    parent_out = None  # --parent-out FILE: its BFS parent row (n x int32 LE)
    profile_out = None  # --profile-out FILE: its level profile, "k reach ecc F h0 ... h_ecc"
    i = 1
    while i < len(argv):
        a = argv[i]
        has = i + 1 < len(argv)
        if a == "-g" and has:
            cfg.graph = argv[i + 1]; i += 1
        elif a == "-q" and has:
            cfg.query = argv[i + 1]; i += 1
        elif a == "-gn" and has:
            cfg.num_gpu = int(argv[i + 1]); i += 1
        elif a == "--algo" and has:
            cfg.algo = argv[i + 1]; i += 1
        elif a == "--gen" and has:
            cfg.gen = argv[i + 1]; i += 1
        elif a == "--qgen" and has:
            cfg.qgen = argv[i + 1]; i += 1
        elif a == "--cache":
            cfg.use_cache = True
        elif a == "--sort-rows":
            cfg.sort_rows = True
        elif a == "--no-relabel":
            cfg.relabel = False
        elif a == "--json":
            json_out = True
            cfg.count_edges = True
        elif a == "--dist-out" and has:
            dist_out = argv[i + 1]; i += 1
        elif a == "--parent-out" and has:
            parent_out = argv[i + 1]; i += 1
        elif a == "--profile-out" and has:
            profile_out = argv[i + 1]; i += 1
        i += 1
    if cfg.num_gpu <= 0:
        print("msbfs: -gn must be >= 1", file=sys.stderr)
        return 1
    import torch
    use_gpu = cfg.algo != "cpu" and torch.cuda.is_available()
    ctx = D.init_from_env(gpus_per_node=cfg.num_gpu, use_gpu=use_gpu)
    eng = Engine(cfg, ctx)
    try:
        eng.preprocess()
    except Exception as e:  # e.g. "Could not open graph file X"
        print(str(e), file=sys.stderr)
        D.shutdown(ctx)
        return 1
    D.barrier(ctx)
    r = eng.compute(gather=json_out)
    if ctx.rank == 0:
        sys.stdout.write(eng.report(r))
        if json_out:
            import json
            print(json.dumps({"K": eng.queries.K, "n": eng.n, "ranks": ctx.world,
                              "backend": ctx.backend, "traversed_edges": r.traversed_edges,
                              "F": [int(x) for x in r.F]}))
        sys.stdout.flush()
        if dist_out is not None or parent_out is not None:
            # after the report, outside the computation time
            row, prow = eng.winner_rows(r, parents=parent_out is not None)
            if row is not None and dist_out is not None:
                row.astype("<i4").tofile(dist_out)
            if prow is not None:
                prow.astype("<i4").tofile(parent_out)
        if profile_out is not None:
            line = eng.winner_profile(r)
            if line is not None:
                with open(profile_out, "w") as f:
                    f.write(line + "\n")
    eng.close()
    D.shutdown(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
