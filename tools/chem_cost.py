#!/usr/bin/env python3
"""What aqueous chemistry costs on bench.py's default box (128^3 cells x 64 super-droplets, fast arithmetic with the lean solver, device
arrays): the trace gases of the kinematic chemistry case, chem_rho 1.8e3, sstp_chem 1.

Per variant -- no chem_switch (the yardstick), chem_switch with the three processes off, all three on, and each alone -- one object after
the other in one process:

  * ms per step of step_sync + step_async, device events on the library's own stream around every step, and the launches and host waits
    of a step (lcx_get_state_u64 "raw_launches");
  * the chemistry substep from the library's own event pair (set_profiling(1), stage "chem": the cell pass, k_chem and the per-cell finish);
  * the substep priced against the bytes it must move per super-droplet: the eight masses read and written, rw2, rd3, n and the two
    words of the sorted order (+ rd3 written with chem_rct; + volume and flag written; chem_dsl: + the six changes written and read again).

There is no target number.

    python tools/chem_cost.py [--n 128] [--steps 10] [--warmup 6] [--out profiles/chem_cost.json]
"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from libcloudphxx_amd import lgrngn  # noqa: E402

M_D = 0.02897
GAS = [.1e-9 * 63e-3 / M_D, .1e-9 * 17e-3 / M_D, 360e-6 * 44e-3 / M_D, .2e-9 * 64e-3 / M_D, .4e-9 * 34e-3 / M_D, 25e-9 * 48e-3 / M_D]
VARIANTS = [("off", ()), ("switch only", ()), ("all", ("chem_dsl", "chem_dsc", "chem_rct")), ("dsl", ("chem_dsl",)), ("dsc", ("chem_dsc",)),
            ("rct", ("chem_rct",)), ("all", ("chem_dsl", "chem_dsc", "chem_rct")), ("off", ())]


def make(n, sd_conc, name, procs, dev):
    oi = bench.make_opts_init(n, n, n, sd_conc, 40., 1, 1, 44)
    oi.strict_fp, oi.cond_solver = False, 0
    opts = lgrngn.opts_t()
    chem = name != "off"
    if chem:
        oi.chem_switch, oi.chem_rho = True, 1.8e3
        for p in procs:
            setattr(opts, p, True)
    prt = lgrngn.factory(lgrngn.backend_t.HIP, oi, np.float64)

    class XP:
        @staticmethod
        def arange(m, dtype=None):
            return torch.arange(m, dtype=torch.float64, device=dev)
        sin, cos, exp, log = staticmethod(torch.sin), staticmethod(torch.cos), staticmethod(torch.exp), staticmethod(torch.log)
    f = bench.make_fields(n, n, n, 0, n, XP, torch.float64)
    shapes = [(n, n, n)] * 3 + [(n + 1, n, n), (n, n + 1, n), (n, n, n + 1)]
    fields = [t.expand(sh).contiguous() for t, sh in zip(f, shapes)]
    arrays = [lgrngn.DeviceArray(t.data_ptr(), t.shape) for t in fields]
    gases = [torch.full((n, n, n), g, dtype=torch.float64, device=dev) for g in GAS] if chem else []
    amb = {lgrngn.chem_species_t(i): lgrngn.DeviceArray(t.data_ptr(), t.shape) for i, t in enumerate(gases)} if chem else None
    torch.cuda.synchronize()
    prt.init(arrays[0], arrays[1], arrays[2], Cx=arrays[3], Cy=arrays[4], Cz=arrays[5], ambient_chem=amb)
    return {"prt": prt, "opts": opts, "keep": (fields, gases), "arrays": arrays, "amb": amb, "stream": torch.cuda.ExternalStream(prt.stream())}


def run_steps(v, k, record):
    prt, opts, a, s = v["prt"], v["opts"], v["arrays"], v["stream"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
    l0 = prt.state_u64("raw_launches").astype(np.int64)
    counts = []
    for i in range(k):
        ev[i].record(s)
        prt.step_sync(opts, a[0], a[1], a[2], a[3], a[4], a[5], ambient_chem=v["amb"])
        prt.step_async(opts)
        l1 = prt.state_u64("raw_launches").astype(np.int64)
        counts.append((l1 - l0).tolist())
        l0 = l1
    ev[k].record(s)
    torch.cuda.synchronize()
    if record is not None:
        for i in range(k):
            record.append((ev[i].elapsed_time(ev[i + 1]), counts[i][0], counts[i][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--sd-conc", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--profiled", type=int, default=4, help="further steps with the library's stage events on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    res = {"box": "%d^3 x %d" % (n, args.sd_conc), "steps": args.steps, "variants": []}
    for name, procs in VARIANTS:
        v = make(n, args.sd_conc, name, procs, dev)
        run_steps(v, args.warmup, None)
        rec = []
        run_steps(v, args.steps, rec)
        ms = np.array([x[0] for x in rec])
        row = {"variant": name, "ms_per_step": float(ms.mean()), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
               "launches_per_step": sorted(set(x[1] for x in rec)), "waits_per_step": sorted(set(x[2] for x in rec)), "n_part": v["prt"].n_part}
        if procs:
            v["prt"].set_profiling(1)
            run_steps(v, args.profiled, None)
            t = v["prt"].timings()
            v["prt"].set_profiling(0)
            row["chem_ms_per_substep"] = t.get("chem", 0.) / args.profiled
            # bytes per super-droplet: masses 8 x 8 B read + written, rw2, rd3, n 8 B each, sorted id + sorted cell 4 B each, volume and flag written
            per = 8 * 8 * 2 + 3 * 8 + 2 * 4 + 2 * 8 + (8 if "chem_rct" in procs else 0) + (6 * 8 * 2 if "chem_dsl" in procs else 0)
            row["bytes_per_droplet"] = per
            if row["chem_ms_per_substep"] > 0:
                row["chem_GB_per_s"] = row["n_part"] * per / (row["chem_ms_per_substep"] * 1e-3) / 1e9
        res["variants"].append(row)
        print(json.dumps(row), flush=True)
        del v
        gc.collect()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
