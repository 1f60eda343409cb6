#!/usr/bin/env python3
"""What a model's output costs: the reference driver's output set written as its loop of classic calls (diag_*_rng, diag_*_mom,
outbuf() per bin and moment) and as one diag_batch() call (include/lcx_diag.h), on bench.py's default box (128^3 cells x 64
super-droplets, double) and on the C2 set-up (76 x 76 x 64, float), a few steps run first.

The request set is kin_cloud_2d_lgrngn.hpp's diag() with the ranges of paper_GMD_2015/fig_a, as numbers: 39 dry bins between 40
edges at a tenth of a decade from 1 nm and 24 wet bins between 25 edges at a fifth of a decade, each at moment 0; the third wet
moment of every dry bin (the driver's "rw3ofrd"); wet moments 0-3 of the cloud range .5-25 um and of the rain range 25 um - 1 m;
sd_conc.  111 requests.

Per box: ms of the whole set (the best of --reps), kernel launches and host waits ("raw_launches"), for the classic loop, the batch
into a host array and the batch into a device array; the batch's bytes per super-droplet and pass, counted from k_diag_batch's
arguments; whether the batch's bits are the loop's.  --classic-only uses only calls that every earlier version of the library has,
so the same tool times the loop on an older build (--lib PATH loads another liblcx_hip.so).  There is no target number.

    python tools/diag_batch_cost.py [--boxes default c2] [--steps 3] [--reps 3] [--classic-only] [--lib PATH] [--out profiles/diag_batch_cost.json]
"""
import argparse
import ctypes as C
import gc
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402
from libcloudphxx_amd import _lib, lgrngn  # noqa: E402


def edge(v):
    return float("%g" % v)                                 # (the driver passes its edges as text of six digits)


def request_set():
    dry = [edge(1e-6 * 10 ** (-3 + i * .1)) for i in range(40)]
    wet = [edge(1e-6 * 10 ** (-3 + i * .2)) for i in range(25)]
    reqs = [([("all",)], ("sd_conc",))]
    reqs += [([("rng", "dry", a, b, False)], ("mom", "dry", 0)) for a, b in zip(dry[:-1], dry[1:])]
    reqs += [([("rng", "wet", .5e-6, 25e-6, False)], ("mom", "wet", k)) for k in range(4)]
    reqs += [([("rng", "wet", 25e-6, 1., False)], ("mom", "wet", k)) for k in range(4)]
    reqs += [([("rng", "wet", a, b, False)], ("mom", "wet", 0)) for a, b in zip(wet[:-1], wet[1:])]
    reqs += [([("rng", "dry", a, b, False)], ("mom", "wet", 3)) for a, b in zip(dry[:-1], dry[1:])]
    return reqs


def classic(prt, reqs, out):
    """the driver's loop, one selection per request as it is written there"""
    for r, (sel, cnt) in enumerate(reqs):
        s = sel[0]
        if s[0] == "all":
            prt.diag_all()
        else:
            getattr(prt, "diag_%s_rng" % s[1])(s[2], s[3])
        if cnt[0] == "sd_conc":
            prt.diag_sd_conc()
        else:
            getattr(prt, "diag_%s_mom" % cnt[1])(cnt[2])
        out[r] = np.frombuffer(prt.outbuf(), dtype=out.dtype)


def timed(prt, torch, f, reps):
    ms, counts = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        l0 = prt.state_u64("raw_launches").astype(np.int64)
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        counts = prt.state_u64("raw_launches").astype(np.int64) - l0
    return {"ms": min(ms), "ms_all": ms, "kernel_launches": int(counts[0]), "host_waits": int(counts[1])}


def make_box(which, lib):
    if which == "c2":
        oi = bench.make_icicle_opts()
        th, rv, rhod, Cx, Cz = bench.make_icicle_fields(dtype=np.float32)
        real_t, fields, kw = np.float32, (th, rv, rhod), {"Cx": Cx, "Cz": Cz}
        name = "C2: 76 x 76 cells x 64, float"
    else:
        n = 128 if which == "default" else int(which)
        oi = bench.make_opts_init(n, n, n, 64, 40., 1, 1, 44)
        oi.strict_fp, oi.cond_solver = False, 0
        th, rv, rhod, Cx, Cy, Cz = bench.make_fields(n, n, n, 0, n, np, np.float64)
        real_t, fields, kw = np.float64, (th, rv, rhod), {"Cx": Cx, "Cy": Cy, "Cz": Cz}
        name = "%d^3 cells x 64, double" % n
    prt = lgrngn.particles_t(oi, real_t, lib=lib)
    prt.init(*fields, **kw)
    return name, prt, real_t, fields, kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", nargs="+", default=["default", "c2"], help="default (bench.py's 128^3), c2, or a number of cells per dimension")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--classic-only", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of liblcx_hip.so")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    lib = C.CDLL(args.lib, mode=C.RTLD_GLOBAL) if args.lib else _lib.load()
    os.environ.setdefault("LCX_DATA_DIR", os.path.join(ROOT, "libcloudphxx_amd", "data"))
    reqs = request_set()
    res = {"host": socket.gethostname(), "lib": args.lib or "in-tree", "requests": len(reqs), "steps_before": args.steps, "reps": args.reps, "boxes": []}
    for which in args.boxes:
        name, prt, real_t, fields, kw = make_box(which, lib)
        opts = lgrngn.opts_t()
        for _ in range(args.steps):
            if which == "c2":
                prt.step_sync(opts, fields[0], fields[1])
            else:
                prt.step_sync(opts, *fields, **kw)
            prt.step_async(opts)
        n_cell, n_part, R = prt.n_cell, prt.n_part, np.dtype(real_t).itemsize
        out_c = np.zeros((len(reqs), n_cell), dtype=real_t)        # (touched: no page faults inside the timed calls)
        classic(prt, reqs[:2], out_c)                              # (warm-up: the sort a first diagnostic pays is not the set's cost)
        row = {"box": name, "n_part": n_part, "n_cell": n_cell, "classic": timed(prt, torch, lambda: classic(prt, reqs, out_c), args.reps)}
        # per (range, moment) the classic kernels move, by their arguments: k_nfilt n, attribute, n_filtered; k_mom_vals sorted_id,
        # n_filtered, attribute, term; k_cell_seqsum term (dead slots and the per-cell arrays left out)
        row["classic"]["bytes_per_droplet_per_request"] = 8 + R + R + 4 + R + R + R + R
        if not args.classic_only:
            rpp, scratch = prt.diag_batch_info()
            out_b = np.zeros_like(out_c)
            prt.diag_batch(reqs[:2], out=out_b[:2])                # (warm-up: the staging areas are allocated once)
            prt.diag_batch(reqs, out=out_b)
            row["batch_host"] = timed(prt, torch, lambda: prt.diag_batch(reqs, out=out_b), args.reps)
            t = torch.zeros((len(reqs), n_cell), dtype=torch.float64 if real_t is np.float64 else torch.float32, device="cuda")
            dev = lgrngn.DeviceArray(t.data_ptr(), (len(reqs), n_cell))
            prt.diag_batch(reqs, out=dev)
            row["batch_device"] = timed(prt, torch, lambda: prt.diag_batch(reqs, out=dev), args.reps)
            passes = -(-len(reqs) // rpp)
            # a pass reads sorted_id, n and the three attributes once per super-droplet (this set uses rd3 and rw2: two)
            row.update(req_per_pass=rpp, passes=passes, scratch_bytes=scratch, batch_bytes_per_droplet_per_pass=4 + 8 + 2 * R,
                       batch_bytes_per_droplet_whole_set=passes * (4 + 8 + 2 * R),
                       classic_bytes_per_droplet_whole_set=len(reqs) * row["classic"]["bytes_per_droplet_per_request"],
                       same_bits_host=bool(np.array_equal(out_b.view(np.uint8), out_c.view(np.uint8))),
                       same_bits_device=bool(np.array_equal(t.cpu().numpy().view(np.uint8), out_c.view(np.uint8))),
                       speedup_host=row["classic"]["ms"] / row["batch_host"]["ms"], speedup_device=row["classic"]["ms"] / row["batch_device"]["ms"])
            del t
        res["boxes"].append(row)
        print(json.dumps(row), flush=True)
        del prt, out_c
        gc.collect()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
