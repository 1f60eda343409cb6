#!/usr/bin/env python3
"""What the budget of tracked super-droplets (include/lcx_track_budget.h) costs, on bench.py's default box (C3: 128^3 cells x 64
super-droplets in double, bench.py's headline options) and on the C2 shape (76 x 76 cells x 64, float, ten condensation and ten
coalescence substeps, host arrays in every step).  Every run is a process of its own (a library is loaded once per process).

  off  C3: this tree's library, budget never enabled, against the parent commit's (--parent-lib PATH), runs alternating, --rounds each:
       3 steps of warm-up, --steps timed steps (wall time around the loop, the device drained before and after).  Gated as
       tools/track_cost.py gates: the medians must lie no further apart than the spread that the parent shows against itself.
  on   per box, set size (1e4 and 1e6 asked for; a box with fewer droplets tracks all it has) and every (0, 1) TWO processes that run the
       same sequence, one with tracking alone and one with the budget as well (a step slows down as the storage drifts from the cell
       order, so two windows of one object cannot be compared), opts_init.reorder_every = 8 so that every window holds re-orderings
       and the scans they cause: warm-up, enable and select, 2 steps, a window of --window timed steps.
       Per window: ms per step, launches per step, `scans`; with the budget also the "track_budget" and "track_sample" stages of a
       profiled stretch of 8 steps behind the window (ms per step: the passes with the scans they pay, the samples with their row
       copies).  --rounds times, alternating; the medians and the spread of the runs with tracking alone are kept beside every run.

    python tools/track_budget_cost.py --parent-lib PATH [--rounds 3] [--steps 20] [--window 24] [--out profiles/track_budget_cost.json]
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
REORDER_EVERY = 8                                                # of the "on" runs: every window holds re-orderings, and so the scans they cause


def one_run(args):
    """a single configuration in this process; prints one JSON line"""
    import numpy as np
    import torch
    import bench
    from libcloudphxx_amd import _lib, lgrngn
    os.environ.setdefault("LCX_DATA_DIR", os.path.join(ROOT, "libcloudphxx_amd", "data"))
    lib = C.CDLL(args.lib, mode=C.RTLD_GLOBAL) if args.lib else _lib.load()
    opts = lgrngn.opts_t()
    if args.box == "c3":
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
        sync = lambda: prt.step_sync(opts, *arrs)
    else:                                                        # bench.c2_leg's object and call
        oi = bench.make_icicle_opts()
        oi.reorder_every = REORDER_EVERY
        th, rv, rhod, Cx, Cz = bench.make_icicle_fields(dtype=np.float32)
        prt = lgrngn.particles_t(oi, np.float32, lib=lib)
        prt.init(th, rv, rhod, Cx=Cx, Cz=Cz)
        sync = lambda: prt.step_sync(opts, th, rv)

    def steps(k):
        for _ in range(k):
            sync()
            prt.step_async(opts)

    def timed(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    launches = lambda: int(prt.state_u64("raw_launches")[0])
    res = {"n_part": int(prt.n_part)}
    steps(3 if args.box == "c3" else 10)
    if args.mode == "step":
        res["ms_per_step"] = timed(args.steps)
        print("RESULT " + json.dumps(res), flush=True)
        return

    prt.track_enable(args.tracked, capacity=256, every=args.every)
    res["n_tracked"] = prt.track_select([("all",)], max_count=args.tracked)
    if args.budget:
        prt.track_budget_enable()
    steps(2)                                                     # (the scan that enable owes, the first sizes of the scratch)
    l0, s0 = launches(), prt.track_info()["scans"]
    res.update(ms_per_step=timed(args.window), launches_per_step=(launches() - l0) / args.window, scans=prt.track_info()["scans"] - s0)
    if args.budget:
        prt.set_profiling(1)
        steps(8)
        torch.cuda.synchronize()
        st = prt.timings()
        prt.set_profiling(0)
        res["stage_track_budget_ms_per_step"] = st.get("track_budget", 0.) / 8
        res["stage_track_sample_ms_per_step"] = st.get("track_sample", 0.) / 8
        res["passes"] = prt.track_budget_info()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblcx_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--window", type=int, default=24)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-off", action="store_true")
    ap.add_argument("--skip-on", action="store_true")
    # a single run (what main starts as child processes)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--box", default="c3", choices=("c3", "c2"))
    ap.add_argument("--mode", default="step", choices=("step", "seq"))
    ap.add_argument("--tracked", type=int, default=0)
    ap.add_argument("--every", type=int, default=0)
    ap.add_argument("--budget", type=int, default=0)
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    res = {"host": socket.gethostname(), "c3": "%d^3 cells x 64, double, bench.py's headline options and default workload" % args.n,
           "c2": "76 x 76 cells x 64, float, sstp_cond = sstp_coal = 10, host arrays (bench.py's c2 leg)", "steps": args.steps, "rounds": args.rounds,
           "window": args.window, "reorder_every_of_on": REORDER_EVERY}

    def run(extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", "--steps", str(args.steps), "--window", str(args.window), "--n", str(args.n)] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        if out.returncode != 0:                                  # (nothing more is started on the device after a run that failed)
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit("a run failed: %s" % " ".join(cmd))
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(" ".join(extra), json.dumps(r), flush=True)
        return r

    ok = True
    if not args.skip_off:
        runs = {"parent": [], "off": []}
        for _ in range(args.rounds):
            if args.parent_lib:
                runs["parent"].append(run(["--lib", args.parent_lib])["ms_per_step"])
            runs["off"].append(run([])["ms_per_step"])
        for name, v in runs.items():
            if v:
                res["off_" + name] = {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
        if runs["parent"]:
            res["off_minus_parent_ms_per_step"] = res["off_off"]["median"] - res["off_parent"]["median"]
            ok = abs(res["off_minus_parent_ms_per_step"]) <= res["off_parent"]["spread"]
            res["off_within_parent_spread"] = ok
    if not args.skip_on:
        for box in ("c3", "c2"):
            for tracked in (10 ** 4, 10 ** 6):
                for every in (0, 1):
                    runs = {0: [], 1: []}
                    for _ in range(args.rounds):
                        for budget in (0, 1):
                            runs[budget].append(run(["--mode", "seq", "--box", box, "--tracked", str(tracked), "--every", str(every), "--budget", str(budget)]))
                    ms = {b: [r["ms_per_step"] for r in runs[b]] for b in runs}
                    res["on_%s_%d_every_%d" % (box, tracked, every)] = {
                        "n_tracked": runs[1][0]["n_tracked"], "tracking_ms_per_step": ms[0], "budget_ms_per_step": ms[1],
                        "budget_minus_tracking_ms_per_step": statistics.median(ms[1]) - statistics.median(ms[0]), "tracking_spread": max(ms[0]) - min(ms[0]),
                        "launches_per_step": [runs[0][0]["launches_per_step"], runs[1][0]["launches_per_step"]], "scans_in_window": runs[1][0]["scans"],
                        "stage_track_budget_ms_per_step": statistics.median(r["stage_track_budget_ms_per_step"] for r in runs[1]),
                        "stage_track_sample_ms_per_step": statistics.median(r["stage_track_sample_ms_per_step"] for r in runs[1]),
                        "passes": runs[1][0]["passes"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
