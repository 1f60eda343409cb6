#!/usr/bin/env python3
"""What a snapshot and a restore cost (include/lcx_state.h) on bench.py's box, 128^3 cells x 64 super-droplets, and on 64^3 x 64: fast
arithmetic with the lean solver, a few steps run first so that the storage carries dead slots and a deferred sort.

Per box, in one process:

  * bytes of the blob and bytes per super-droplet;
  * ms of lcx_snapshot_save into a host buffer that has been touched before (pageable, as a caller's is), and of lcx_snapshot_load into
    a fresh object -- each next to a plain hipMemcpy of equally many bytes from the device to the same pageable buffer and back;
  * the checksum pass alone (both launches, device events): ms and GB/s over as many bytes as the blob holds.

There is no target number.

    python tools/snapshot_cost.py [--n 64 128] [--steps 6] [--reps 3] [--out profiles/snapshot_cost.json]
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


def chk(lib, rc):
    if rc != 0:
        lib.lcx_last_error.restype = C.c_char_p
        raise RuntimeError(lib.lcx_last_error().decode())


def make(n, sd_conc):
    oi = bench.make_opts_init(n, n, n, sd_conc, 40., 1, 1, 44)
    oi.strict_fp, oi.cond_solver = False, 0
    return oi


def bare_copy(lib, host, reps):
    """hipMemcpy of len(host) bytes: device -> pageable host, pageable host -> device; ms, the best of `reps`"""
    dev = C.c_void_p()
    chk(lib, lib.lcx_dev_alloc(C.byref(dev), C.c_size_t(host.size)))
    d2h, h2d = [], []
    try:
        for _ in range(reps):
            chk(lib, lib.lcx_dev_sync())
            t0 = time.perf_counter()
            chk(lib, lib.lcx_dev_copy(C.c_void_p(host.ctypes.data), dev, C.c_size_t(host.size), C.c_int(2)))
            chk(lib, lib.lcx_dev_sync())
            t1 = time.perf_counter()
            chk(lib, lib.lcx_dev_copy(dev, C.c_void_p(host.ctypes.data), C.c_size_t(host.size), C.c_int(1)))
            chk(lib, lib.lcx_dev_sync())
            t2 = time.perf_counter()
            d2h.append((t1 - t0) * 1e3)
            h2d.append((t2 - t1) * 1e3)
    finally:
        chk(lib, lib.lcx_dev_free(dev))
    return min(d2h), min(h2d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--sd-conc", type=int, default=64)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    res = {"host": socket.gethostname(), "steps_before": args.steps, "reps": args.reps, "boxes": []}
    for n in args.n:
        oi = make(n, args.sd_conc)
        th, rv, rhod, Cx, Cy, Cz = bench.make_fields(n, n, n, 0, n, np, np.float64)
        prt = lgrngn.factory(lgrngn.backend_t.HIP, oi, np.float64)
        prt.init(th, rv, rhod, Cx=Cx, Cy=Cy, Cz=Cz)
        opts = lgrngn.opts_t()
        for _ in range(args.steps):
            prt.step_sync(opts, th, rv, rhod, Cx=Cx, Cy=Cy, Cz=Cz)
            prt.step_async(opts)
        size = C.c_size_t()
        chk(lib, lib.lcx_snapshot_size(prt._h, C.byref(size)))
        host = np.zeros(size.value, dtype=np.uint8)               # (touched: no page faults inside the timed calls)
        storage = len(prt.state_u64("raw_n"))
        save = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            chk(lib, lib.lcx_snapshot_save(prt._h, C.c_void_p(host.ctypes.data), C.c_size_t(host.size), C.byref(size)))
            save.append((time.perf_counter() - t0) * 1e3)
        n_part = prt.n_part
        del prt
        gc.collect()
        load = []
        for _ in range(args.reps):
            q = lgrngn.factory(lgrngn.backend_t.HIP, oi, np.float64)
            t0 = time.perf_counter()
            chk(lib, lib.lcx_snapshot_load(q._h, C.c_void_p(host.ctypes.data), C.c_size_t(size.value)))
            load.append((time.perf_counter() - t0) * 1e3)
            del q
            gc.collect()
        d2h, h2d = bare_copy(lib, host, args.reps)
        ms = C.c_double()
        chk(lib, lib.lcx_snapshot_checksum_time(C.c_size_t(size.value), C.c_int(10), C.byref(ms)))
        row = {"box": "%d^3 x %d" % (n, args.sd_conc), "n_part": n_part, "storage": storage, "blob_bytes": size.value,
               "bytes_per_droplet": size.value / storage, "snapshot_ms": min(save), "snapshot_ms_all": save, "restore_ms": min(load),
               "restore_ms_all": load, "hipMemcpy_d2h_ms": d2h, "hipMemcpy_h2d_ms": h2d, "snapshot_over_copy": min(save) / d2h,
               "restore_over_copy": min(load) / h2d, "checksum_ms": ms.value, "checksum_GB_per_s": size.value / (ms.value * 1e-3) / 1e9}
        res["boxes"].append(row)
        print(json.dumps(row), flush=True)
        del host
        gc.collect()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
