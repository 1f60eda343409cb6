#!/usr/bin/env python3
"""What the aerosol source costs on bench.py's default box (128^3 cells x 64 super-droplets, fast arithmetic with the lean solver,
device arrays): ms per step of step_sync + step_async

  (a) without a source,
  (b) src_type = simple in the lowest 4 planes, 8 super-droplets per cell, supstp 1, 10 and 1000 (= one firing, in the warm-up),
  (c) the same with src_type = matching,

all in ONE process, the variants taking turns in chunks of steps, device events on the library's own stream around every step, so
that firing and non-firing steps are told apart.  The whole round is run twice (`pass`): the spread of the run itself.  There is no
target number: the yardstick is (a) from the same run.

    python tools/source_cost.py [--n 128] [--steps 130] [--warmup 10] [--out profiles/source_cost.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from libcloudphxx_amd import lgrngn  # noqa: E402

PLANES, SD_PER_CELL = 4, 8
SRC = lgrngn.lognormal(.05e-6, 1.4, 60e4 / 100)      # per second; a hundredth of the reference test's rate (the box is run for minutes)


def make(n, sd_conc, variant, steps_total, dev):
    src_type, supstp = variant
    oi = bench.make_opts_init(n, n, n, sd_conc, 40., 1, 1, 44)
    oi.strict_fp, oi.cond_solver = False, 0
    opts = lgrngn.opts_t()
    if src_type != "off":
        oi.src_type = lgrngn.src_t[src_type]
        oi.src_x1 = oi.src_y1 = n * 40.
        oi.src_z1 = PLANES * 40.
        per_firing = n * n * PLANES * SD_PER_CELL
        # simple grows at every firing; matching needs the room for one firing's candidates and saturates
        oi.n_sd_max += per_firing * ((steps_total + supstp - 1) // supstp + 1 if src_type == "simple" else 4)
        opts.src = True
        opts.src_dry_distros = {(.61, 0.): (SRC, SD_PER_CELL, supstp)}
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
            "supstp": supstp, "src_type": src_type, "n_part_start": prt.n_part}


def run_chunk(v, k, record):
    prt, opts, a, s = v["prt"], v["opts"], v["arrays"], v["stream"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
    l0 = prt.state_u64("raw_launches").astype(np.int64)
    waits = []
    for i in range(k):
        ev[i].record(s)
        prt.step_sync(opts, a[0], a[1], a[2], a[3], a[4], a[5])
        prt.step_async(opts)
        l1 = prt.state_u64("raw_launches").astype(np.int64)
        waits.append((l1 - l0).tolist())
        l0 = l1
    ev[k].record(s)
    torch.cuda.synchronize()
    for i in range(k):
        fires = v["src_type"] != "off" and v["step"] % v["supstp"] == 0
        if record is not None:
            record.append((fires, ev[i].elapsed_time(ev[i + 1]), waits[i][0], waits[i][1]))
        v["step"] += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--sd-conc", type=int, default=64)
    ap.add_argument("--steps", type=int, default=130, help="timed steps per variant and pass")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    # (supstp 1000: fires once, in the warm-up -- the control that tells what the source's code path costs a non-firing step from what
    # the super-droplets it has added cost)
    variants = [("off", 1), ("simple", 1), ("simple", 10), ("simple", 1000), ("matching", 1), ("matching", 10), ("matching", 1000)]
    total = args.warmup + args.passes * args.steps
    objs = [make(args.n, args.sd_conc, v, total, dev) for v in variants]
    for v in objs:
        run_chunk(v, args.warmup, None)
    res = {"box": "%d^3 x %d" % (args.n, args.sd_conc), "source": "lowest %d planes, %d super-droplets per cell" % (PLANES, SD_PER_CELL),
           "steps_per_pass": args.steps, "passes": []}
    for _ in range(args.passes):
        recs = [[] for _ in objs]
        for _ in range(args.steps // args.chunk):
            for v, r in zip(objs, recs):
                run_chunk(v, args.chunk, r)
        row = {}
        for (src_type, supstp), v, r in zip(variants, objs, recs):
            ms = np.array([x[1] for x in r])
            fire = np.array([x[0] for x in r], dtype=bool)
            behind = np.concatenate([[False], fire[:-1]]) & ~fire
            row["%s/%d" % (src_type, supstp)] = {
                "ms_per_step": float(ms.mean()), "timed_ms": float(ms.sum()),
                "ms_firing_step": float(ms[fire].mean()) if fire.any() else None,
                "ms_other_step": float(ms[~fire].mean()) if (~fire).any() else None,
                # the step behind a firing apart from the rest of the non-firing steps (it starts from another state of the sort)
                "ms_step_behind_firing": float(ms[behind].mean()) if behind.any() else None,
                "ms_later_steps": float(ms[~fire & ~behind].mean()) if (~fire & ~behind).any() else None,
                "launches_firing_step": float(np.mean([x[2] for x in r if x[0]])) if fire.any() else None,
                "waits_firing_step": float(np.mean([x[3] for x in r if x[0]])) if fire.any() else None,
                "launches_other_step": float(np.mean([x[2] for x in r if not x[0]])) if (~fire).any() else None,
                "waits_other_step": float(np.mean([x[3] for x in r if not x[0]])) if (~fire).any() else None,
                "n_part_start": v["n_part_start"], "n_part_now": v["prt"].n_part}
        res["passes"].append(row)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
