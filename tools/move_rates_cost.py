#!/usr/bin/env python3
"""What the move rates (include/lcx_move_rates.h) cost: configurations on one box in one session, by turns -- the parent commit's
library (--parent-lib PATH), this tree's library with the tally off, and with it on at [25 um], at [0] (every droplet) and at three
thresholds (0, 25 and 60 um) -- on bench.py's default workload, 128^3 cells x 64 super-droplets in double, bench.py's headline options.

Every run is a process of its own (a library is loaded once per process): 3 steps of warm-up, --steps timed steps (wall time around
the loop, the device drained before and after), then 4 steps with every stage's events on for the "move(adve+sedi+bcnd)" and
"move_rates" rows of the stage table.  The "on" configurations run twice: on freshly re-ordered storage (opts_init.reorder_every = 1) and
on storage that has drifted (reorder_every = 10000 and 40 steps of warm-up: the timed window sees no re-ordering).  The rounds go parent,
off, on..., parent, ...; per configuration the result holds every round's numbers, their median and their spread (max - min).  "Off" is
gated: its median must lie no further from the parent's median than the spread that the parent shows against itself (off must be the
parent's step); the result says so in "off_within_parent_spread" and the tool exits with 1 where it does not.  "On" is reported.

--regs TREE [TREE ...] needs no GPU: it compiles csrc/lcx_core.hip of each tree to device assembly and lists the registers, scratch, LDS
and argument bytes of every k_move instantiation (they must be the parent's: no move kernel is touched) and of the tally kernels.

    python tools/move_rates_cost.py --parent-lib PATH [--rounds 3] [--steps 30] [--n 128] [--out profiles/move_rates_cost.json]
    python tools/move_rates_cost.py --regs . ../parent [--merge profiles/move_rates_cost.json] [--out ...]
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
THRESHOLDS = {"none": None, "rain": [25e-6], "all": [0.], "three": [0., 25e-6, 60e-6]}
KEYS = ("ms_per_step", "move_ms_per_step", "move_rates_ms_per_step")


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
    if args.storage == "fresh":
        oi.reorder_every = 1
    elif args.storage == "drifted":
        oi.reorder_every = 10000
    shapes = [(n, n, n)] * 3 + [(n + 1, n, n), (n, n + 1, n), (n, n, n + 1)]
    f = [torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, sh))).to("cuda") for a, sh in zip(bench.make_fields(n, n, n, 0, n, np, np.float64), shapes)]
    torch.cuda.synchronize()
    arrs = [lgrngn.DeviceArray(t.data_ptr(), t.shape) for t in f]
    prt = lgrngn.particles_t(oi, np.float64, lib=lib)
    prt.init(arrs[0], arrs[1], arrs[2], Cx=arrs[3], Cy=arrs[4], Cz=arrs[5])
    thr = THRESHOLDS[args.tally]
    if thr is not None:
        prt.move_rates_enable(thr)
    opts = lgrngn.opts_t()

    def steps(k):
        for _ in range(k):
            prt.step_sync(opts, *arrs)
            prt.step_async(opts)
    steps(40 if args.storage == "drifted" else 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps(args.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    prt.set_profiling(1)
    steps(4)
    torch.cuda.synchronize()
    st = prt.timings()
    res = {"ms_per_step": ms, "move_ms_per_step": st.get("move(adve+sedi+bcnd)", 0.) / 4, "move_rates_ms_per_step": st.get("move_rates", 0.) / 4,
           "n_part": int(prt.n_part)}
    if thr is not None:
        res["calls_tallied"] = prt.move_rates_info()[2]
        prt.move_rates(reset=True)
        steps(1)
        got = prt.move_rates()
        res["rows_of_one_step"] = {k: [float(x) for x in np.atleast_2d(v).sum(1)] for k, v in got.items() if k.endswith("_n")}
    print("RESULT " + json.dumps(res), flush=True)


def kernel_table(tree):
    """{kernel: [vgpr, sgpr, scratch bytes, LDS bytes, argument bytes]} of the move and tally kernels of a tree"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result", "--cuda-device-only",
                               "-S", os.path.join(tree, "libcloudphxx_amd", "csrc", "lcx_core.hip"), "-o", out])
        text = open(out).read()
    meta = text[text.rfind("amdhsa.kernels"):]
    for chunk in meta.split("\n  - "):
        m = re.search(r"\n\s+\.name:\s+(_Z\S*k_move\S*)\n", "\n" + chunk)
        if not m:
            continue
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", chunk).group(1))
        name = m.group(1)
        if filt:
            name = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void lcx::", "")
        table[name] = [g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), g("kernarg_segment_size")]
    return {"kernels": table, "global_atomic_add_f64": text.count("global_atomic_add_f64")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblcx_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", nargs="+", default=None, help="run these configurations only (names of the result's \"order\")")
    ap.add_argument("--regs", nargs="+", default=None, help="trees whose move kernels' registers to list (no GPU)")
    ap.add_argument("--merge", default=None, help="with --regs: a result file of the timing mode to add the tables to")
    # a single run (what the rounds start as child processes)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tally", default="none", choices=sorted(THRESHOLDS))
    ap.add_argument("--storage", default="default", choices=("default", "fresh", "drifted"))
    args = ap.parse_args()
    if args.one:
        return one_run(args)
    if args.regs:
        res = json.load(open(args.merge)) if args.merge else {}
        res["registers"] = {os.path.abspath(t) == ROOT and "this" or "parent": kernel_table(t) for t in args.regs}
        ok = True
        if "this" in res["registers"] and "parent" in res["registers"]:
            mine, theirs = res["registers"]["this"]["kernels"], res["registers"]["parent"]["kernels"]
            new = lambda k: "k_move_rates" in k                                                   # (the tally and its read-out)
            ok = theirs == {k: v for k, v in mine.items() if not new(k)}
            res["registers"]["move_kernels_equal_parent"] = ok
        line = json.dumps(res)
        print(line)
        if args.out:
            open(args.out, "w").write(line + "\n")
        return 0 if ok else 1
    configs = [("parent", args.parent_lib, "none", "default"), ("off", None, "none", "default")]
    for storage in ("fresh", "drifted"):
        configs += [("off_" + storage, None, "none", storage)] + [("on_%s_%s" % (t, storage), None, t, storage) for t in ("rain", "all", "three")]
    if not args.parent_lib:
        configs = configs[1:]
    if args.only:
        configs = [c for c in configs if c[0] in args.only]
    res = {"host": socket.gethostname(), "box": "%d^3 cells x 64, double, bench.py's headline options and default workload" % args.n, "steps": args.steps,
           "rounds": args.rounds, "order": [c[0] for c in configs], "thresholds": {k: v for k, v in THRESHOLDS.items() if v}}
    runs = {c[0]: [] for c in configs}
    for _ in range(args.rounds):
        for name, lib, tally, storage in configs:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "--tally", tally, "--storage", storage, "--steps", str(args.steps), "--n", str(args.n)]
            if lib:
                cmd += ["--lib", lib]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:                             # (nothing more is started on the device after a run that failed)
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit("a run failed: %s" % " ".join(cmd))
            r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            runs[name].append(r)
            print(name, json.dumps(r), flush=True)
    summary = {}
    for name, rs in runs.items():
        summary[name] = {"runs": rs}
        for key in KEYS:
            v = [r[key] for r in rs]
            summary[name][key] = {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    ok = True
    for name in runs:
        base = "off_" + name.rsplit("_", 1)[1] if name.startswith("on_") else None
        if base in summary:
            for key in KEYS[:2]:
                summary[name + "_minus_" + base + "_" + key] = summary[name][key]["median"] - summary[base][key]["median"]
    if "parent" in summary and "off" in summary:
        p = summary["parent"]["ms_per_step"]
        summary["off_minus_parent_ms_per_step"] = summary["off"]["ms_per_step"]["median"] - p["median"]
        ok = abs(summary["off"]["ms_per_step"]["median"] - p["median"]) <= p["spread"]
        summary["off_within_parent_spread"] = ok
    res.update(summary)
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
