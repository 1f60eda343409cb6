#!/usr/bin/env python3
"""What the collision log (include/lcx_coal_log.h) costs: five configurations on one box in one session, by turns -- the parent commit's
library (--parent-lib PATH), this tree's library with everything off, with the collision rates on at 25 um (the TALLY forms as they
were before the log), with the log on at r_min = 0 and with the log on at r_min = 25 um -- on bench.py's default workload and on its
colliding one, 128^3 cells x 64 super-droplets in double, bench.py's headline options.

Every run is a process of its own (a library is loaded once per process): 3 steps of warm-up, --steps timed steps (wall time around
the loop, the device drained before and after, no read of the log in between), then 4 steps with every stage's events on for the
"coal" row of the stage table.  The rounds go parent, off, rates, log0, log25, parent, ...; per configuration the result holds every
round's numbers, their median and their spread (max - min).  "Off against parent" is read against the spread that the alternating runs
of the two show; the "on" configurations are reported, not gated.  A log run also reports seen, held and the capacity: once the list is
full the kernels go on counting (the atomic per wave) but store nothing.

--regs TREE PARENT needs no GPU: it compiles csrc/lcx_core.hip of each tree to device assembly and lists the registers, scratch, LDS
and argument bytes of every coalescence kernel (tools/coal_rates_cost.py's table): the TALLY = false forms must be the parent's, and
what the TALLY = true forms gained is listed beside the occupancy step (waves per SIMD by VGPRs) of both.

    python tools/coal_log_cost.py --parent-lib PATH [--rounds 3] [--steps 20] [--n 128] [--out profiles/coal_log_cost.json]
    python tools/coal_log_cost.py --regs . ../parent [--merge profiles/coal_log_cost.json] [--out ...]
"""
import argparse
import ctypes as C
import json
import os
import re
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coal_rates_cost import kernel_table  # noqa: E402  (the same listing, of the same kernels)

R_25 = 25e-6
CAPACITY = 1 << 22
# name -> (library, coal_rates on, log's r_min or None)
CONFIGS = [("parent", "parent", False, None), ("off", None, False, None), ("rates", None, True, None), ("log0", None, False, 0.), ("log25", None, False, R_25)]


def one_run(args):
    """a single configuration in this process; prints one JSON line"""
    import numpy as np
    import torch
    import bench
    from libcloudphxx_amd import _lib, lgrngn
    os.environ.setdefault("LCX_DATA_DIR", os.path.join(ROOT, "libcloudphxx_amd", "data"))
    lib = C.CDLL(args.lib, mode=C.RTLD_GLOBAL) if args.lib else _lib.load()
    n = args.n
    oi = bench.make_opts_init(n, n, n, 64, 40., 1, 1, 44, workload=args.workload)
    oi.strict_fp, oi.cond_solver = False, 0
    shapes = [(n, n, n)] * 3 + [(n + 1, n, n), (n, n + 1, n), (n, n, n + 1)]
    f = [torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, sh))).to("cuda") for a, sh in zip(bench.make_fields(n, n, n, 0, n, np, np.float64), shapes)]
    torch.cuda.synchronize()
    arrs = [lgrngn.DeviceArray(t.data_ptr(), t.shape) for t in f]
    prt = lgrngn.particles_t(oi, np.float64, lib=lib)
    prt.init(arrs[0], arrs[1], arrs[2], Cx=arrs[3], Cy=arrs[4], Cz=arrs[5])
    if args.rates:
        prt.coal_rates_enable(R_25)
    if args.r_min >= 0:
        prt.coal_log_enable(args.capacity, args.r_min)
    opts = lgrngn.opts_t()

    def steps(k):
        for _ in range(k):
            prt.step_sync(opts, *arrs)
            prt.step_async(opts)
    steps(3)
    if args.r_min >= 0:
        prt.coal_log_enable(args.capacity, args.r_min)          # (emptied: the timed steps start with all the room)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps(args.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    res = {"ms_per_step": ms, "n_part": int(prt.n_part)}
    if args.r_min >= 0:
        _, cap, r_min, held, seen, launches = prt.coal_log_info()
        res.update({"capacity": cap, "r_min": r_min, "held": held, "seen": seen, "launches": launches, "seen_per_step": seen / args.steps})
    prt.set_profiling(1)
    steps(4)
    torch.cuda.synchronize()
    res["coal_ms_per_step"] = prt.timings().get("coal", 0.) / 4
    res["coal_kernel"], res["coal_ranked"] = int(prt.state_u64("raw_coal_kernel")[0]), int(prt.state_u64("raw_coal_ranked")[0])
    print("RESULT " + json.dumps(res), flush=True)


def waves_by_vgprs(vgprs):
    """waves per SIMD that a kernel's VGPR count allows on gfx950 (512 VGPRs per lane and SIMD, allocated in blocks of 8, at most 8 waves)"""
    return max(1, min(8, 512 // max(8, (vgprs + 7) // 8 * 8)))


def tally(name):
    """whether a kernel's name is a TALLY = true form: the last template parameter of k_coal and k_coal_cells, the fifth of the six of
    k_coal_ranked<T, MARK, SKIP, EXIT, TALLY, TILES>"""
    if "<" not in name:
        return False
    params = name[name.index("<") + 1:name.rindex(">")].split(", ")
    at = 4 if "k_coal_ranked<" in name and len(params) == 6 else len(params) - 1
    return params[at] == "true"


def regs(args):
    res = json.load(open(args.merge)) if args.merge else {}
    mine, theirs = kernel_table(args.regs[0]), kernel_table(args.regs[1])
    return regs_report(args, res, mine, theirs)


def regs_report(args, res, mine, theirs):
    new = lambda k: "k_coal_log" in k                                                        # (the two kernels of the read path)
    off_mine = {k: v for k, v in mine["kernels"].items() if not tally(k) and not new(k)}
    off_theirs = {k: v for k, v in theirs["kernels"].items() if not tally(k)}
    gained = {}
    for k, v in mine["kernels"].items():
        if tally(k) and k in theirs["kernels"]:
            p = theirs["kernels"][k]
            gained[k] = {"parent": p, "this": v, "delta": [a - b for a, b in zip(v, p)], "waves_parent": waves_by_vgprs(p[0]), "waves_this": waves_by_vgprs(v[0])}
    res["registers"] = {"columns": ["vgpr", "sgpr", "scratch bytes", "LDS bytes", "argument bytes"], "this": mine, "parent": theirs,
                        "tally_false_forms_equal_parent": off_mine == off_theirs and len(off_mine) > 0,
                        "tally_false_forms": len(off_mine), "tally_true_forms": gained,
                        "tally_true_forms_crossing_an_occupancy_step": sorted(k for k, g in gained.items() if g["waves_parent"] != g["waves_this"]),
                        "read_path": {k: v for k, v in mine["kernels"].items() if new(k)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblcx_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--capacity", type=int, default=CAPACITY)
    ap.add_argument("--out", default=None)
    ap.add_argument("--regs", nargs=2, default=None, metavar=("TREE", "PARENT"), help="the two trees whose coalescence kernels' registers to list (no GPU)")
    ap.add_argument("--merge", default=None, help="with --regs: a result file of the timing mode to add the tables to")
    # a single run (what the rounds start as child processes)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rates", type=int, default=0)
    ap.add_argument("--r-min", type=float, default=-1., help="the log's r_min; negative: the log stays off")
    ap.add_argument("--workload", default="stratocumulus", choices=["stratocumulus", "coal-stress"])
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    if args.regs:
        return regs(args)
    configs = [c for c in CONFIGS if c[1] is None or args.parent_lib]
    res = {"host": socket.gethostname(), "box": "%d^3 cells x 64, double, bench.py's headline options" % args.n, "steps": args.steps, "rounds": args.rounds,
           "capacity": args.capacity, "order": [c[0] for c in configs], "workloads": {}}
    for workload in ("stratocumulus", "coal-stress"):
        runs = {c[0]: [] for c in configs}
        for _ in range(args.rounds):
            for name, lib, rates, r_min in configs:
                cmd = [sys.executable, os.path.abspath(__file__), "--one", "--workload", workload, "--rates", str(int(rates)), "--steps", str(args.steps),
                       "--n", str(args.n), "--capacity", str(args.capacity), "--r-min", str(-1. if r_min is None else r_min)]
                if lib:
                    cmd += ["--lib", args.parent_lib]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:                             # (nothing more is started on the device after a run that failed)
                    sys.stderr.write(out.stdout + out.stderr)
                    raise SystemExit("a run failed: %s" % " ".join(cmd))
                r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
                runs[name].append(r)
                print(workload, name, json.dumps(r), flush=True)
        summary = {}
        for name, rs in runs.items():
            summary[name] = {"runs": rs}
            for key in ("ms_per_step", "coal_ms_per_step"):
                v = [r[key] for r in rs]
                summary[name][key] = {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
        for key in ("ms_per_step", "coal_ms_per_step"):
            med = lambda name: summary[name][key]["median"]
            if "parent" in summary:
                summary["off_minus_parent_" + key] = med("off") - med("parent")
                summary["spread_off_and_parent_" + key] = max(summary["off"][key]["spread"], summary["parent"][key]["spread"])
            for name in ("rates", "log0", "log25"):
                summary[name + "_minus_off_" + key] = med(name) - med("off")
            for name in ("log0", "log25"):
                summary[name + "_minus_rates_" + key] = med(name) - med("rates")
        res["workloads"][workload] = summary
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
