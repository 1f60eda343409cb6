#!/usr/bin/env python3
"""What tracked super-droplets (include/lcx_track.h) cost, on bench.py's default workload: 128^3 cells x 64 super-droplets in double,
bench.py's headline options.  Every run is a process of its own (a library is loaded once per process).

  a   off: this tree's library against the parent commit's (--parent-lib PATH), runs alternating, --rounds each: 3 steps of warm-up,
      --steps timed steps (wall time around the loop, the device drained before and after).  Gated: the medians must lie no further apart
      than the spread that the parent shows against itself ("off_within_parent_spread"; the tool exits with 1 where they do not).
  b-f one process per set size (1e4 and 1e6 tracked) and one without tracking that runs the same sequence, all with
      opts_init.reorder_every = 8 so that the timed windows hold re-orderings:
      f   track_select over the whole box (wall time of the call, which waits for the stream; its launches)
      b   enabled, nothing sampled: ms per step over 24 steps and the "reorder_storage" stage's ms per re-ordering, beside the run without
      c   a sample on unpermuted storage: wall time of track_sample + a drain of the stream, median of 10; launches per sample; `scans`
      d   a sample behind a permutation (the step that re-orders): the same, once; launches; `scans`
      e   every = 1 over 100 steps against the run without

    python tools/track_cost.py --parent-lib PATH [--rounds 3] [--steps 20] [--n 128] [--out profiles/track_cost.json]
"""
import argparse
import ctypes as C
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REORDER_EVERY = 8


def one_run(args):
    """a single configuration in this process; prints one JSON line"""
    import numpy as np
    import torch
    import bench
    from libcloudphxx_amd import _lib, lgrngn
    os.environ.setdefault("LCX_DATA_DIR", os.path.join(ROOT, "libcloudphxx_amd", "data"))
    lib = C.CDLL(args.lib, mode=C.RTLD_GLOBAL) if args.lib else _lib.load()
    n = args.n
    oi = bench.make_opts_init(n, n, n, 64, 40., 1, 1, 44, workload="stratocumulus")
    oi.strict_fp, oi.cond_solver = False, 0
    if args.mode != "step":
        oi.reorder_every = REORDER_EVERY
    shapes = [(n, n, n)] * 3 + [(n + 1, n, n), (n, n + 1, n), (n, n, n + 1)]
    f = [torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, sh))).to("cuda") for a, sh in zip(bench.make_fields(n, n, n, 0, n, np, np.float64), shapes)]
    torch.cuda.synchronize()
    arrs = [lgrngn.DeviceArray(t.data_ptr(), t.shape) for t in f]
    prt = lgrngn.particles_t(oi, np.float64, lib=lib)
    prt.init(arrs[0], arrs[1], arrs[2], Cx=arrs[3], Cy=arrs[4], Cz=arrs[5])
    opts = lgrngn.opts_t()
    done = [0]

    def steps(k):
        for _ in range(k):
            prt.step_sync(opts, *arrs)
            prt.step_async(opts)
        done[0] += k

    def timed(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    launches = lambda: int(prt.state_u64("raw_launches")[0])
    res = {"n_part": int(prt.n_part)}
    if args.mode == "step":                                      # item a
        steps(3)
        res["ms_per_step"] = timed(args.steps)
        print("RESULT " + json.dumps(res), flush=True)
        return
    tracked = args.tracked
    steps(3)
    if tracked:
        prt.track_enable(tracked, capacity=128)
        torch.cuda.synchronize()
        n0, t0 = launches(), time.perf_counter()
        got = prt.track_select([("all",)], max_count=tracked)
        res["f_select_ms"], res["f_select_launches"], res["n_tracked"] = (time.perf_counter() - t0) * 1e3, launches() - n0, got
    # b: 24 steps = three re-orderings, nothing sampled; then the stage table of 8 more steps (one re-ordering)
    res["b_ms_per_step"] = timed(24)
    prt.set_profiling(1)
    steps(8)
    torch.cuda.synchronize()
    st = prt.timings()
    prt.set_profiling(0)
    res["b_reorder_storage_ms"] = st.get("reorder_storage", 0.)
    res["b_post_copy_ms_per_step"] = st.get("post_copy", 0.) / 8
    if tracked:
        # c: unpermuted storage (steps 36, 37 of a period of 8: the next re-ordering is step 40's)
        steps(1)
        prt.track_sample()                                       # (the one behind the last re-ordering: scan + sample)
        torch.cuda.synchronize()
        scans0, ts, ls = prt.track_info()["scans"], [], []
        for _ in range(10):
            n0, t0 = launches(), time.perf_counter()
            prt.track_sample()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            ls.append(launches() - n0)
        res["c_sample_ms"], res["c_sample_ms_min"], res["c_launches"] = statistics.median(ts), min(ts), ls
        res["c_scans_added"] = prt.track_info()["scans"] - scans0
        # d: behind a permutation
        while done[0] % REORDER_EVERY != REORDER_EVERY - 3 % REORDER_EVERY:
            steps(1)
        steps(3)                                                 # (three more: the re-ordering is among them wherever the period began)
        torch.cuda.synchronize()
        scans0, n0, t0 = prt.track_info()["scans"], launches(), time.perf_counter()
        prt.track_sample()
        torch.cuda.synchronize()
        res["d_sample_ms"], res["d_launches"], res["d_scans_added"] = (time.perf_counter() - t0) * 1e3, launches() - n0, prt.track_info()["scans"] - scans0
        prt.track(reset=True)
        prt.track_enable(tracked, capacity=128, every=1)         # e: start over with every = 1
        prt.track_select([("all",)], max_count=tracked)
    res["e_ms_per_step_100"] = timed(100)
    if tracked:
        info = prt.track_info()
        res["e_samples"], res["e_scans"], res["e_dropped"] = info["n_samples"], info["scans"], info["dropped"]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblcx_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-bf", action="store_true")
    # a single run (what main starts as child processes)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--mode", default="step", choices=("step", "seq"))
    ap.add_argument("--tracked", type=int, default=0)
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    res = {"host": socket.gethostname(), "box": "%d^3 cells x 64, double, bench.py's headline options and default workload" % args.n, "steps": args.steps,
           "rounds": args.rounds, "reorder_every_of_b_to_f": REORDER_EVERY}

    def run(extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", "--steps", str(args.steps), "--n", str(args.n)] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        if out.returncode != 0:                                  # (nothing more is started on the device after a run that failed)
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit("a run failed: %s" % " ".join(cmd))
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(" ".join(extra), json.dumps(r), flush=True)
        return r

    ok = True
    if not args.skip_a:
        runs = {"parent": [], "off": []}
        for _ in range(args.rounds):
            if args.parent_lib:
                runs["parent"].append(run(["--lib", args.parent_lib])["ms_per_step"])
            runs["off"].append(run([])["ms_per_step"])
        for name, v in runs.items():
            if v:
                res["a_" + name] = {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
        if runs["parent"]:
            res["a_off_minus_parent_ms_per_step"] = res["a_off"]["median"] - res["a_parent"]["median"]
            ok = abs(res["a_off_minus_parent_ms_per_step"]) <= res["a_parent"]["spread"]
            res["off_within_parent_spread"] = ok
    if not args.skip_bf:
        res["seq_off"] = run(["--mode", "seq"])
        for tracked in (10 ** 4, 10 ** 6):
            res["seq_on_%d" % tracked] = run(["--mode", "seq", "--tracked", str(tracked)])
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
