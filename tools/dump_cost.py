#!/usr/bin/env python3
"""What the particle dump (include/lcx_dump.h) costs, on bench.py's default workload: 128^3 cells x 64 super-droplets in double, bench.py's
headline options, after --spin-up steps.  Every run is a process of its own (a library is loaded once per process).

  a   no dump issued: this tree's library against the parent commit's (--parent-lib PATH), runs alternating, --rounds each: 3 steps of
      warm-up, --steps timed steps (wall time around the loop, the device drained before and after).  Gated: the medians must lie no
      further apart than the spread that the parent shows against itself ("off_within_parent_spread"; the tool exits with 1 where not).
  b   one process with this tree's library.  Wall time of each call with the device drained before it (the call waits for the stream
      itself), median and minimum of --reps, and its launches:
      count     the count-only call of the rain selection in the sub-box, and of every droplet: the mark pass, the scan, the read-back
      1 rain    wet radius >= --r-rain in a column of 8 x 8 cells, seven fields, to the host (a box without rain yet: the threshold is
                lowered by tenths until a thousand droplets of the column lie above it; "r_rain_used")
      2 all     every droplet, seven fields, into a device array
      3 strided every droplet with max_count = 1e6, seven fields, to the host; and into a device array (the call without the link)
      and the copy rate of the box (a device-to-device copy of one 1.07 GB column, bytes read + written per second), from which the
      model of each pass follows: mark = (n + the clause's columns + the box's positions) / rate; gather = n_storage / 8 bytes + 2 x 8 bytes
      x fields x taken, at that rate.
  c   what a caller has without the call, in a process with the parent's library where given (this tree's otherwise: lcx_get_attr is
      unchanged): six get_attr calls + state_u64("n") for the multiplicity + the numpy filter of the rain selection on the host.

    python tools/dump_cost.py --parent-lib PATH [--rounds 3] [--steps 20] [--n 128] [--out profiles/dump_cost.json]
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
FIELDS = ("n", "x", "y", "z", "rw2", "rd3", "kappa")


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
    shapes = [(n, n, n)] * 3 + [(n + 1, n, n), (n, n + 1, n), (n, n, n + 1)]
    f = [torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, sh))).to("cuda") for a, sh in zip(bench.make_fields(n, n, n, 0, n, np, np.float64), shapes)]
    torch.cuda.synchronize()
    arrs = [lgrngn.DeviceArray(t.data_ptr(), t.shape) for t in f]
    prt = lgrngn.particles_t(oi, np.float64, lib=lib)
    prt.init(arrs[0], arrs[1], arrs[2], Cx=arrs[3], Cy=arrs[4], Cz=arrs[5])
    opts = lgrngn.opts_t()

    def steps(k):
        for _ in range(k):
            prt.step_sync(opts, *arrs)
            prt.step_async(opts)

    launches = lambda: int(prt.state_u64("raw_launches")[0])
    res = {"n_part": int(prt.n_part)}
    if args.mode == "step":                                      # item a
        steps(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(args.steps)
        torch.cuda.synchronize()
        res["ms_per_step"] = (time.perf_counter() - t0) / args.steps * 1e3
        print("RESULT " + json.dumps(res), flush=True)
        return
    steps(args.spin_up)
    torch.cuda.synchronize()
    dx = 40.
    box = (0., 8 * dx, 0., 8 * dx, 0., n * dx)
    r_rain = args.r_rain
    if args.mode != "step" and hasattr(lib, "lcx_dump"):         # a box that holds no rain yet: the threshold comes down until the sub-box
        while prt.dump_count([("rng", "wet", r_rain, 1.)], box=box) < 1000 and r_rain > 1e-7:      # holds a thousand droplets above it
            r_rain *= .9
    elif args.r_used:
        r_rain = args.r_used
    res["r_rain_used"] = r_rain
    rain = [("rng", "wet", r_rain, 1.)]

    def timed(call, reps):
        ts, ls, out = [], [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            n0, t0 = launches(), time.perf_counter()
            out = call()
            ts.append((time.perf_counter() - t0) * 1e3)
            ls.append(launches() - n0)
        return {"ms_median": statistics.median(ts), "ms_min": min(ts), "launches": ls[-1]}, out

    if args.mode == "today":                                     # item c
        def today():
            cols = {nm: prt.get_attr(nm) for nm in ("rw2", "rd3", "kappa", "x", "y", "z")}
            cols["n"] = prt.state_u64("n")
            t1 = time.perf_counter()
            keep = (cols["rw2"] >= r_rain ** 2) & (cols["x"] >= box[0]) & (cols["x"] < box[1]) & (cols["y"] >= box[2]) & (cols["y"] < box[3])
            sel = {nm: v[keep] for nm, v in cols.items()}
            return int(keep.sum()), (time.perf_counter() - t1) * 1e3, sum(v.nbytes for v in cols.values())
        r, (q, filt_ms, nbytes) = timed(today, max(args.reps // 2, 1))
        res["c_today"] = dict(r, n_selected=q, of_which_numpy_filter_ms=filt_ms, bytes_to_host=nbytes)
        print("RESULT " + json.dumps(res), flush=True)
        return
    # item b
    n_storage = int(prt.state_u64("raw_n").size)
    res["n_storage"] = n_storage
    a, b_ = torch.empty(n_storage, dtype=torch.float64, device="cuda"), torch.empty(n_storage, dtype=torch.float64, device="cuda")
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b_.copy_(a)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    rate = 2 * 8 * n_storage / min(ts)
    del a, b_
    res["copy_rate_GBps"] = rate / 1e9
    r, q = timed(lambda: prt.dump_count(rain, box=box), args.reps)
    res["count_rain"] = dict(r, Q=q, model_ms=(8 + 8 + 3 * 8) * n_storage / rate * 1e3, model_n_and_rw2_only_ms=(8 + 8) * n_storage / rate * 1e3)
    r, q_all = timed(lambda: prt.dump_count(), args.reps)
    res["count_all"] = dict(r, Q=q_all, model_ms=8 * n_storage / rate * 1e3)
    r, d = timed(lambda: prt.dump(rain, box=box, fields=FIELDS, max_count=max(q, 1)), args.reps)
    res["1_rain"] = dict(r, Q=d["n_qualifying"], n_written=int(d["n"].size),
                         model_ms=((8 + 8 + 3 * 8) * n_storage + n_storage / 8 + 2 * 8 * len(FIELDS) * d["n"].size) / rate * 1e3)
    out = torch.empty((len(FIELDS), q_all), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    r, d = timed(lambda: prt.dump(fields=FIELDS, max_count=q_all, out=lgrngn.DeviceArray(out.data_ptr(), out.shape)), args.reps)
    res["2_all_device"] = dict(r, Q=d["n_qualifying"], n_written=d["n_written"],
                               model_ms=(8 * n_storage + n_storage / 8 + 2 * 8 * len(FIELDS) * d["n_written"]) / rate * 1e3)
    assert int(out[0].min().item()) >= 1, "every multiplicity written is positive"
    del out
    r, d = timed(lambda: prt.dump(fields=FIELDS, max_count=10 ** 6), args.reps)
    res["3_all_strided"] = dict(r, Q=d["n_qualifying"], stride=d["stride"], n_written=int(d["n"].size),
                                model_ms=(8 * n_storage + n_storage / 8 + 2 * 8 * len(FIELDS) * d["n"].size) / rate * 1e3)
    out = torch.full((len(FIELDS), 10 ** 6), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    r, d = timed(lambda: prt.dump(fields=FIELDS, max_count=10 ** 6, out=lgrngn.DeviceArray(out.data_ptr(), out.shape)), args.reps)
    res["3_all_strided_device"] = dict(r, Q=d["n_qualifying"], stride=d["stride"], n_written=d["n_written"], model_ms=res["3_all_strided"]["model_ms"])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblcx_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--spin-up", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--r-rain", type=float, default=25e-6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-bc", action="store_true")
    # a single run (what main starts as child processes)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--mode", default="step", choices=("step", "dump", "today"))
    ap.add_argument("--r-used", type=float, default=0., help="(today, with a library that has no dump) the threshold that the dump run settled on")
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    res = {"host": socket.gethostname(), "box": "%d^3 cells x 64, double, bench.py's headline options and default workload" % args.n, "steps": args.steps,
           "rounds": args.rounds, "spin_up": args.spin_up, "reps": args.reps, "r_rain": args.r_rain, "fields": list(FIELDS)}

    def run(extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", "--steps", str(args.steps), "--n", str(args.n), "--spin-up", str(args.spin_up),
               "--reps", str(args.reps), "--r-rain", repr(args.r_rain)] + extra
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
    if not args.skip_bc:
        res["b_dump"] = run(["--mode", "dump"])
        res["c_today"] = run(["--mode", "today", "--r-used", repr(res["b_dump"]["r_rain_used"])] + (["--lib", args.parent_lib] if args.parent_lib else []))
        res["c_library"] = "parent" if args.parent_lib else "this tree"
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
