#!/usr/bin/env python3
"""What the collision rates (include/lcx_coal_rates.h) cost: three builds on one box in one session, by turns -- the parent commit's
library (--parent-lib PATH), this tree's library with the accumulators off, and with them on -- on bench.py's default workload and on
its colliding one (the "coalescence that collides" leg: the Golovin test's spectrum under hall_davis_no_waals), 128^3 cells x 64
super-droplets in double, bench.py's headline options.

Every run is a process of its own (a library is loaded once per process): 3 steps of warm-up, --steps timed steps (wall time around
the loop, the device drained before and after), then 4 steps with every stage's events on for the "coal" row of the stage table (the
coalescence launches of a step).  The rounds go parent, off, on, parent, off, on ...; per configuration the result holds every round's
numbers, their median and their spread (max - min), so that "off against parent" can be read against the spread that the parent shows
against itself.  "On" is reported, not gated.

--regs TREE [TREE ...] needs no GPU: it compiles csrc/lcx_core.hip of each tree to device assembly and lists the registers, scratch,
LDS and argument bytes of every coalescence kernel (the TALLY = false forms must be the parent's).

    python tools/coal_rates_cost.py --parent-lib PATH [--rounds 3] [--steps 30] [--n 128] [--out profiles/coal_rates_cost.json]
    python tools/coal_rates_cost.py --regs . ../parent [--out ...]
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import socket
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R_THR = 25e-6


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
    if args.tally:
        prt.coal_rates_enable(R_THR)
    opts = lgrngn.opts_t()

    def steps(k):
        for _ in range(k):
            prt.step_sync(opts, *arrs)
            prt.step_async(opts)
    steps(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps(args.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    prt.set_profiling(1)
    steps(4)
    torch.cuda.synchronize()
    st = prt.timings()
    res = {"ms_per_step": ms, "coal_ms_per_step": st.get("coal", 0.) / 4, "n_part": int(prt.n_part),
           "coal_kernel": int(prt.state_u64("raw_coal_kernel")[0]), "coal_ranked": int(prt.state_u64("raw_coal_ranked")[0])}
    if args.tally:
        got = prt.coal_rates()
        res["launches_tallied"] = prt.coal_rates_info()[2]
        res["events_last_window"] = {k: float(v.sum()) for k, v in got.items()}
    print("RESULT " + json.dumps(res), flush=True)


def kernel_table(tree):
    """{kernel: [vgpr, sgpr, scratch bytes, LDS bytes, argument bytes]} of the coalescence kernels of a tree's lcx_core.hip"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "core.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result", "--cuda-device-only",
                               "-S", os.path.join(tree, "libcloudphxx_amd", "csrc", "lcx_core.hip"), "-o", out])
        text = open(out).read()
    meta = text[text.rfind("amdhsa.kernels"):]
    table = {}
    for chunk in meta.split("\n  - "):
        m = re.search(r"\n\s+\.name:\s+(_Z\S*k_coal\S*)\n", "\n" + chunk)
        if not m:
            continue
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", chunk).group(1))
        name = m.group(1)
        if filt:
            name = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void lcx::", "")
        table[name] = [g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), g("kernarg_segment_size")]
    return {"kernels": table, "cmpswap_loops": text.count("cmpswap"), "global_atomic_add_f64": text.count("global_atomic_add_f64")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblcx_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--regs", nargs="+", default=None, help="trees whose coalescence kernels' registers to list (no GPU)")
    ap.add_argument("--merge", default=None, help="with --regs: a result file of the timing mode to add the tables to")
    # a single run (what the rounds start as child processes)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tally", type=int, default=0)
    ap.add_argument("--workload", default="stratocumulus", choices=["stratocumulus", "coal-stress"])
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    if args.regs:
        res = json.load(open(args.merge)) if args.merge else {}
        res["registers"] = {os.path.abspath(t) == ROOT and "this" or "parent": kernel_table(t) for t in args.regs}
        if "this" in res["registers"] and "parent" in res["registers"]:
            mine, theirs = res["registers"]["this"]["kernels"], res["registers"]["parent"]["kernels"]
            off = {k: v for k, v in mine.items() if not k.rstrip(">").endswith("true")}       # (TALLY is the last parameter)
            same = {re.sub(r", false>$", ">", k): v[:4] for k, v in off.items()}
            new = lambda k: "k_coal_rate" in k                                                    # (the two kernels of the read path)
            res["registers"]["tally_false_forms_equal_parent"] = {k: v[:4] for k, v in theirs.items()} == {k: v for k, v in same.items() if not new(k)}
        line = json.dumps(res)
        print(line)
        if args.out:
            open(args.out, "w").write(line + "\n")
        return
    configs = [("parent", args.parent_lib, 0), ("off", None, 0), ("on", None, 1)]
    if not args.parent_lib:
        configs = configs[1:]
    res = {"host": socket.gethostname(), "box": "%d^3 cells x 64, double, bench.py's headline options" % args.n, "steps": args.steps, "rounds": args.rounds,
           "order": [c[0] for c in configs], "workloads": {}}
    for workload in ("stratocumulus", "coal-stress"):
        runs = {c[0]: [] for c in configs}
        for _ in range(args.rounds):
            for name, lib, tally in configs:
                cmd = [sys.executable, os.path.abspath(__file__), "--one", "--workload", workload, "--tally", str(tally), "--steps", str(args.steps), "--n", str(args.n)]
                if lib:
                    cmd += ["--lib", lib]
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
            if "parent" in summary:
                summary["off_minus_parent_" + key] = summary["off"][key]["median"] - summary["parent"][key]["median"]
            summary["on_minus_off_" + key] = summary["on"][key]["median"] - summary["off"][key]["median"]
        res["workloads"][workload] = summary
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
