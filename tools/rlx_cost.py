#!/usr/bin/env python3
"""What aerosol relaxation costs on bench.py's default box (128^3 cells x 64 super-droplets, fast arithmetic with the lean solver,
device arrays): one spectrum (twice the initial one), rlx_sd_per_bin 1, the lowest quarter of the levels, a firing every 10 steps
with a time scale long enough that every firing creates its super-droplets.

Per variant -- the census with the per-level table in LDS at rlx_bins 64, 256 and 1024 (the cap), and the census with one global
atomic per droplet (opts_init.dbg_flags RLX_GLOBAL_ATOMICS) at rlx_bins 1024 -- one object after the other in one process:

  * ms per step of step_sync + step_async, device events on the library's own stream around every step: firing steps against the
    other steps of the same run, and launches / host waits of both;
  * the stages of a firing from the library's own event pairs (set_profiling(1)): rlx_census (ONE launch), rlx_plan (plan + scan),
    rlx_create (the newcomers and what every new super-droplet gets); what is left of the difference is the read-back's wait;
  * the census priced against its bytes: the droplets of the relaxed levels x (n 8 B + rd3 8 B + sorted id 4 B [+ kappa 8 B]).

The variant "off" (no rlx_switch) is the yardstick of the non-firing steps.  There is no target number.

    python tools/rlx_cost.py [--n 128] [--steps 40] [--warmup 12] [--out profiles/rlx_cost.json]
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

SUPSTP = 10
TARGET = lgrngn.lognormal([.02e-6, .075e-6], [1.4, 1.6], [120e6, 80e6])      # twice bench.py's initial spectrum


def make(n, sd_conc, variant, dev):
    census, bins = variant
    oi = bench.make_opts_init(n, n, n, sd_conc, 40., 1, 1, 44)
    oi.strict_fp, oi.cond_solver = False, 0
    opts = lgrngn.opts_t()
    if census != "off":
        oi.rlx_switch = True
        oi.rlx_bins, oi.rlx_sd_per_bin, oi.rlx_timescale, oi.supstp_rlx = bins, 1, 1e4, SUPSTP
        oi.rlx_dry_distros = {.61: [TARGET, [0, 2], [0, (n // 4) * 40.]]}
        if census == "global":
            oi.dbg_flags |= int(lgrngn.dbg.RLX_GLOBAL_ATOMICS)
        opts.rlx = True
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
    torch.cuda.synchronize()
    prt.init(arrays[0], arrays[1], arrays[2], Cx=arrays[3], Cy=arrays[4], Cz=arrays[5])
    return {"prt": prt, "opts": opts, "fields": fields, "arrays": arrays, "stream": torch.cuda.ExternalStream(prt.stream()), "step": 0,
            "on": census != "off", "n_part_start": prt.n_part}


def run_steps(v, k, record):
    prt, opts, a, s = v["prt"], v["opts"], v["arrays"], v["stream"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
    l0 = prt.state_u64("raw_launches").astype(np.int64)
    counts = []
    for i in range(k):
        ev[i].record(s)
        prt.step_sync(opts, a[0], a[1], a[2], a[3], a[4], a[5])
        prt.step_async(opts)
        l1 = prt.state_u64("raw_launches").astype(np.int64)
        counts.append((l1 - l0).tolist())
        l0 = l1
    ev[k].record(s)
    torch.cuda.synchronize()
    for i in range(k):
        fires = v["on"] and v["step"] % SUPSTP == 0
        if record is not None:
            record.append((fires, ev[i].elapsed_time(ev[i + 1]), counts[i][0], counts[i][1]))
        v["step"] += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--sd-conc", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40, help="timed steps per variant (a firing every 10)")
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--profiled", type=int, default=20, help="further steps with the library's stage events on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    # (the headline variant and the yardstick twice: the spread and the drift of a box that warms up over the run)
    # (a LCX_RLX_MAX_BINS raised for the occasion takes ("lds", 2048), ("lds", 4096) as well: profiles/rlx_cost.json has them)
    variants = [("off", 0), ("lds", 1024), ("global", 1024), ("lds", 64), ("lds", 256), ("lds", 1024), ("lds", 64), ("off", 0)]
    n, quarter = args.n, args.n // 4
    res = {"box": "%d^3 x %d" % (n, args.sd_conc), "relaxed": "lowest %d of %d levels, one spectrum, rlx_sd_per_bin 1, supstp_rlx %d" % (quarter, n, SUPSTP),
           "steps": args.steps, "variants": []}
    for census, bins in variants:
        v = make(n, args.sd_conc, (census, bins), dev)
        run_steps(v, args.warmup - args.warmup % SUPSTP + SUPSTP if v["on"] else args.warmup, None)       # (ends on a multiple of supstp_rlx)
        rec = []
        run_steps(v, args.steps, rec)
        ms = np.array([x[1] for x in rec])
        fire = np.array([x[0] for x in rec], dtype=bool)
        row = {"census": census, "rlx_bins": bins, "ms_per_step": float(ms.mean()),
               "ms_firing_step": float(ms[fire].mean()) if fire.any() else None, "ms_firing_steps": ms[fire].tolist(),
               "ms_other_step": float(ms[~fire].mean()), "sd_other_step": float(ms[~fire].std(ddof=1)),
               "launches_firing_step": [x[2] for x in rec if x[0]], "waits_firing_step": [x[3] for x in rec if x[0]],
               "launches_other_step": sorted(set(x[2] for x in rec if not x[0])), "waits_other_step": sorted(set(x[3] for x in rec if not x[0])),
               "n_part_start": v["n_part_start"], "n_part_now": v["prt"].n_part}
        if v["on"]:
            v["prt"].set_profiling(1)
            run_steps(v, args.profiled - args.profiled % SUPSTP, None)
            t = v["prt"].timings()
            firings = (args.profiled - args.profiled % SUPSTP) // SUPSTP
            row["stage_ms_per_firing"] = {k: t[k] / firings for k in ("rlx_census", "rlx_plan", "rlx_create") if k in t}
            v["prt"].set_profiling(0)
            # bytes the census has to read: the droplets of the relaxed levels (n, rd3, the sorted id; kappa is one value in this run)
            # LDS form: n, rd3 and the sorted id that leads to them; global-atomic form: n, rd3 and ijk, in storage order
            per = 8 + 8 + 4
            droplets = v["n_part_start"] * (quarter / n if census == "lds" else 1.)
            row["census_droplets"] = droplets
            row["census_bytes_per_droplet"] = per
            if "rlx_census" in row["stage_ms_per_firing"]:
                row["census_GB_per_s"] = droplets * per / (row["stage_ms_per_firing"]["rlx_census"] * 1e-3) / 1e9
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
