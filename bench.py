#!/usr/bin/env python3
"""bench.py -- super-droplets/s of the lgrngn time step (step_sync + step_async: condensation,
coalescence, advection, sedimentation, boundary, re-sort) on the BASELINE workload:
3-D stratocumulus-like box 128^3 cells x 64 super-droplets per cell (BASELINE.json configs[2]).

    python bench.py --gpus 1 --steps 200 --warmup 5
    python bench.py --gpus N ...                      # ONE process, N devices: the native multi_HIP object (lcx_create_multi)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W        # one process per GPU: libcloudphxx_amd/multi.py, migrants over RCCL
                                                      # (--native: rank 0 drives all N devices with the native object instead)

A "step" is one full pass of the hot path over all super-droplets.  Inputs (th, rv, rhod, Courant numbers) are
device-resident when the timed region starts (N > 1: every slab's planes on its own device).  Rank 0 prints ONE JSON line.
N > 1: the SAME box is split into N slabs along x (strong scaling, as BASELINE.json's metric asks: one problem at 1/2/4/8
GPUs); super-droplets that cross a slab face are handed to the neighbouring device (no collective).
--oversubscribe maps all N slabs to device 0 (what a one-GPU box can measure of the N-slab protocol).

A plain run sets up, warms up, times --steps steps and prints the headline line (metric, value, unit, ms_per_step, dtype, config).
--full adds everything else this script measures: the roofline and the stage table (their own hipEvents and extra steps), the device's
copy bandwidth, the legs (other arithmetic, host arrays, coal-stress, soak, activation, C2, C5) and the CPU baseline.
--dump-outputs DIR writes the caller's th and rv after the last timed step as DIR/th.npy and DIR/rv.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.3 TB/s achievable)


def bimodal():
    from libcloudphxx_amd import lgrngn
    # icicle's aerosol, models/kinematic_2D/src/opts_common.hpp:56-62
    return lgrngn.lognormal([.02e-6, .075e-6], [1.4, 1.6], [60e6, 40e6])


def make_opts_init(nx, ny, nz, sd_conc, dx, sstp_cond, sstp_coal, seed, workload="stratocumulus", dt=1., kernel=None):
    from libcloudphxx_amd import lgrngn
    oi = lgrngn.opts_init_t()
    oi.nx, oi.ny, oi.nz = nx, ny, nz
    oi.dx = oi.dy = oi.dz = dx
    oi.x1, oi.y1, oi.z1 = nx * dx, ny * dx, nz * dx
    oi.dt = dt
    oi.sd_conc = sd_conc
    oi.n_sd_max = int(nx * ny * nz * sd_conc * 1.15) + 1024
    if workload == "coal-stress":
        # SURVEY 8(d), C5 variant (ii): the exponential-in-volume spectrum of the reference's Golovin test (tests/python/physics/
        # coalescence_golovin.py:31-44,68-74: r_zero = 30.084 um, n_zero = 2^23 per m^3, kappa = 1e-10) under a gravitational kernel
        # with tabulated efficiencies -- drizzle-sized drops that DO collide (a per cent of the candidate pairs per second)
        oi.dry_distros = {(1e-10, 0.): lgrngn.expvolume(30.084e-6, 2 ** 23)}
        oi.kernel = lgrngn.kernel_t[kernel] if kernel else lgrngn.kernel_t.hall_davis_no_waals
    else:
        oi.dry_distros = {(.61, 0.): bimodal()}
        oi.kernel = lgrngn.kernel_t[kernel] if kernel else lgrngn.kernel_t.hall_pinsky_stratocumulus   # (init fails loudly if its efficiency table is missing)
    oi.terminal_velocity = lgrngn.vt_t.beard77fast
    oi.adve_scheme = lgrngn.as_t.euler
    oi.sstp_cond, oi.sstp_coal = sstp_cond, sstp_coal
    oi.rng_seed = seed
    return oi


def make_icicle_opts(nx=76, nz=76, sd_conc=64, sstp=10):
    """BASELINE configs[1] (C2): the 2-D kinematic icicle set-up of the GMD 2015 paper -- 76 x 76 cells of 20 m, 64 super-droplets per cell,
    ten condensation and ten coalescence substeps, the geometric kernel x 0.5, khvorostyanov_spherical terminal velocities, implicit
    advection (ref models/kinematic_2D/src/opts_lgrngn.hpp:262,340-343, kin_cloud_2d_lgrngn.hpp:167-170, tests/paper_GMD_2015/fig_a/calc.cpp:36-39)"""
    from libcloudphxx_amd import lgrngn
    dx = 1500. / 75
    oi = lgrngn.opts_init_t()
    oi.nx, oi.ny, oi.nz = nx, 0, nz
    oi.dx = oi.dz = dx
    oi.dy = 1.
    oi.x0, oi.z0 = dx / 2, dx / 2
    oi.x1, oi.z1 = (nx - .5) * dx, (nz - .5) * dx
    oi.y1 = 1.
    oi.dt = 1.
    oi.sd_conc = sd_conc
    oi.n_sd_max = int(sd_conc * nx * nz * 1.2)
    oi.dry_distros = {(.61, 0.): bimodal()}
    oi.kernel = lgrngn.kernel_t.geometric
    oi.kernel_parameters = [0.5]
    oi.terminal_velocity = lgrngn.vt_t.khvorostyanov_spherical
    oi.adve_scheme = lgrngn.as_t.implicit
    oi.sstp_cond = oi.sstp_coal = sstp
    return oi


def make_icicle_fields(nx=76, nz=76, dtype=np.float32):
    """th = 289 K, rv = 7.5e-3, rhod(z); the single-eddy stream function with w_max = 0.6 m/s (ref models/kinematic_2D/cases/
    icmw8_case1.hpp:166-228): air rises through cloud base in one half of the domain in every step"""
    dx = 1500. / 75
    X, Z = nx * dx, nz * dx
    z = (np.arange(nz) + .5) * dx
    rhod = np.broadcast_to(1.2 * np.exp(-z / 8000.), (nx, nz)).astype(dtype).copy()
    th = np.full((nx, nz), 289., dtype=dtype)
    rv = np.full((nx, nz), 7.5e-3, dtype=dtype)
    A = 0.6 * X / (2 * np.pi)
    xe, ze = np.arange(nx + 1) * dx, np.arange(nz + 1) * dx
    xc, zc = (np.arange(nx) + .5) * dx, (np.arange(nz) + .5) * dx
    u = -A * np.pi / Z * np.cos(np.pi * zc[None, :] / Z) * np.cos(2 * np.pi * xe[:, None] / X)
    w = A * 2 * np.pi / X * np.sin(np.pi * ze[None, :] / Z) * np.sin(2 * np.pi * xc[:, None] / X)
    return th, rv, rhod, np.ascontiguousarray((u / dx / 1.2).astype(dtype)), np.ascontiguousarray((w / dx / 1.2).astype(dtype))


def make_fields(nx_loc, ny, nz, x_off, nx_tot, xp, dtype):
    """th, rv, rhod and a smooth non-divergent-ish Courant field with |C| <= 0.3 for the slab of x-planes
    [x_off, x_off + nx_loc).  xp is numpy (CPU sample) or torch-on-device."""
    def idx(shape, axis, off=0.):
        n = shape[axis]
        v = xp.arange(n, dtype=dtype) + off
        sh = [1, 1, 1]
        sh[axis] = n
        return v.reshape(sh)
    two_pi = 2 * np.pi
    s = (nx_loc, ny, nz)
    z = idx(s, 2, .5) / nz
    th = 289. + 0. * z + 0.2 * xp.sin(two_pi * (idx(s, 0, x_off) / nx_tot)) * xp.cos(two_pi * idx(s, 1) / ny)
    rhod = 1.1 - 0.02 * z + 0. * th
    # rv from a target relative humidity: 0.85 at the bottom rising to 1.015 in the upper third (activation + growth)
    R_d, R_v, c_pd = 8.3144621 / 0.02897, 8.3144621 / 0.018, 1005.
    T = (th * (rhod * R_d / 1e5) ** (R_d / c_pd)) ** (c_pd / (c_pd - R_d))
    p_vs = 611.73 * xp.exp((2.5e6 + (4218. - 1850.) * 273.16) / R_v * (1. / 273.16 - 1. / T) - (4218. - 1850.) / R_v * xp.log(T / 273.16))
    RH_t = 0.85 + 0.25 * z
    RH_t = RH_t - (RH_t - 1.015) * (RH_t > 1.015)
    rv = RH_t * p_vs / (rhod * R_v * T)
    sx, sy, sz = (nx_loc + 1, ny, nz), (nx_loc, ny + 1, nz), (nx_loc, ny, nz + 1)
    Cx = 0.3 * xp.sin(two_pi * idx(sx, 1, .5) / ny) * xp.cos(np.pi * idx(sx, 2, .5) / nz) + 0. * idx(sx, 0)
    Cy = 0.2 * xp.sin(two_pi * (idx(sy, 0, x_off + .5) / nx_tot)) + 0. * idx(sy, 1) + 0. * idx(sy, 2)
    Cz = 0.1 * xp.sin(two_pi * (idx(sz, 0, x_off + .5) / nx_tot)) * xp.sin(np.pi * idx(sz, 2) / nz) + 0. * idx(sz, 1)
    return [a.contiguous() if hasattr(a, "contiguous") else np.ascontiguousarray(a) for a in (th, rv, rhod, Cx, Cy, Cz)]


def host_cpu():
    """model string and physical core count of the host (printed next to the CPU baseline)"""
    model, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif not line.strip():
                if core is not None:
                    cores.add((phys, core))
                phys = core = None
    except OSError:
        pass
    return model, len(cores) or (os.cpu_count() or 1)


def mem_available_gb():
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable"):
                return int(ln.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.


def cpu_baseline(args):
    """the CPU oracle (a port of the reference path; OpenMP on its elementwise loops, stable sort, per-cell counts and sums, the way the
    reference's thrust::omp backend spreads them; the Mersenne-Twister draws stay serial as the reference's are) timed on a bounded
    sample of the same workload: the headline box itself, a few steps"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _harness as h
    from libcloudphxx_amd import lgrngn
    n = args.cpu_sample_n
    note = ""
    need_gb = 45. * (n / 128.) ** 3 * (args.sd_conc / 64.)           # the oracle's ~35 per-SD arrays of 8 bytes + sort work space
    if mem_available_gb() < 1.5 * need_gb and n > 64:
        note = " (host memory %.0f GB: sample reduced from %d^3)" % (mem_available_gb(), n)
        n = 64
    oi = make_opts_init(n, n, n, args.sd_conc, args.dx, args.sstp_cond, args.sstp_coal, 44, args.workload, args.dt, args.kernel)
    th, rv, rhod, Cx, Cy, Cz = make_fields(n, n, n, 0, n, np, np.float64)
    lib = h.oracle_omp_lib()
    quota = h.cpu_quota()                                           # (oracle_omp_lib has already set the thread count to it)
    threads = int(lib.orc_num_threads())
    pr = h.oracle_omp_particles(oi)
    model, phys = host_cpu()
    pr.init(th, rv, rhod, Cx=Cx, Cy=Cy, Cz=Cz)
    opts = lgrngn.opts_t()
    pr.step_sync(opts, th, rv, rhod, Cx, Cy, Cz)
    pr.step_async(opts)
    t0 = time.perf_counter()
    done = 0
    for _ in range(args.cpu_sample_steps):
        pr.step_sync(opts, th, rv, rhod, Cx, Cy, Cz)
        pr.step_async(opts)
        done += pr.n_part
    dt = time.perf_counter() - t0
    return {"value": done / dt, "unit": "super-droplets/s", "cores": threads, "kind": "port",
            "cpu_model": model, "physical_cores": phys, "cpu_quota": quota,
            "sample": "%d^3 cells x %d SD/cell%s, %d full steps (cond+coal+adve+sedi) after one warm-up step, C oracle with OpenMP "
                      "(elementwise loops, sort, per-cell sums; serial generator) on %d threads = the CPUs this process is granted "
                      "(%s, %d physical cores in the box), %.1f s" % (n, args.sd_conc, note, args.cpu_sample_steps, threads, model, phys, dt),
            # the reference's OWN OpenMP backend, timed during the survey in the build container: the anchor
            # that says what reference code does per core; the port above is what can run on the GPU box
            "reference_openmp_anchor": {"value": 2.56e6, "unit": "super-droplets/s", "cores": 8, "kind": "reference",
                                        "sample": "the reference's thrust::omp backend, 64^3-class box, build container, BASELINE.md section 2"}}


DUMP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, seed=1234):
    """writes {name: float32 / float64 array} as out_dir/<name>.npy.  If together they would hold more than DUMP_BYTES, every array is cut
    to a sample of its flattened elements, in ascending index order, that depends only on the seed and its size: two runs with the
    same arguments write the same elements (the headline box's th and rv, 2 x 16.8 MB, are written whole)"""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        if total > DUMP_BYTES:
            keep = max(1, a.size * DUMP_BYTES // total)
            a = a.reshape(-1)[np.sort(np.random.default_rng(seed).choice(a.size, keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def c2_leg(lgrngn, torch, steps=60, warmup=10, real_t=np.float32, **change):
    """BASELINE configs[1] timed: 76 x 76 cells x 64 super-droplets, sstp 10 / 10, float, icicle's call (th, rv as host arrays in every
    step).  3.7e5 super-droplets and twenty substeps: what a step costs here is its launches and host waits, so both are counted"""
    oi = make_icicle_opts()
    for k, v in change.items():
        setattr(oi, k, v)
    th, rv, rhod, Cx, Cz = make_icicle_fields(dtype=real_t)
    pr = lgrngn.factory(lgrngn.backend_t.HIP, oi, real_t)
    pr.init(th, rv, rhod, Cx=Cx, Cz=Cz)
    opts = lgrngn.opts_t()
    for _ in range(warmup):
        pr.step_sync(opts, th, rv)
        pr.step_async(opts)
    torch.cuda.synchronize()
    l0 = pr.state_u64("raw_launches")
    t0 = time.perf_counter()
    done = 0
    for _ in range(steps):
        pr.step_sync(opts, th, rv)
        pr.step_async(opts)
        done += pr.n_part
    torch.cuda.synchronize()
    dt_ = time.perf_counter() - t0
    l1 = pr.state_u64("raw_launches")
    return {"value": done / dt_, "unit": "super-droplets/s", "ms_per_step": dt_ / steps * 1e3, "steps": steps,
            "kernel_launches_per_step": float(l1[0] - l0[0]) / steps, "host_waits_per_step": float(l1[1] - l0[1]) / steps,
            "super_droplets": int(done / steps), "dtype": "f32" if real_t == np.float32 else "f64",
            "workload": "2-D kinematic icicle set-up (BASELINE configs[1]): 76 x 76 cells x 64 SD/cell, sstp_cond = sstp_coal = 10, geometric kernel x 0.5, "
                        "khvorostyanov_spherical, implicit advection, the API's default arithmetic (cond_solver = 1), th and rv as host arrays in every step"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=128, help="cells per dimension (BASELINE: 128)")
    ap.add_argument("--nx", type=int, default=0, help="override the number of x-planes (emulates one slab of a decomposed run)")
    ap.add_argument("--ny", type=int, default=0, help="override the number of cells in y (C4: --nx 256 --ny 256 --nz 128)")
    ap.add_argument("--nz", type=int, default=0, help="override the number of cells in z")
    ap.add_argument("--sd-conc", type=int, default=64)
    ap.add_argument("--dx", type=float, default=40.)
    ap.add_argument("--sstp-cond", type=int, default=1)
    ap.add_argument("--sstp-coal", type=int, default=1)
    ap.add_argument("--cond-mode", choices=["percell", "pp_nomix", "pp_adaptive", "pp_mix"], default="percell",
                    help="condensation substepping: per cell (default) or per particle (exact_sstp_cond) without mixing / "
                         "adaptive / with mixing; only meaningful with --sstp-cond > 1")
    ap.add_argument("--real", choices=["f64", "f32"], default="f64")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong")
    ap.add_argument("--strict-fp", action="store_true",
                    help="IEEE operation order in the condensation kernel and the reference's TOMS748 iterates (the API default); default "
                         "here: fast arithmetic -- the collected one-division growth rate with FMA under the lean bracketed secant")
    ap.add_argument("--cond-solver", choices=["lean", "toms748"], default="lean",
                    help="fast arithmetic only (opts_init.cond_solver): the lean bracketed secant, or the reference's TOMS748 iterates in "
                         "fast arithmetic (round 2's kernels)")
    ap.add_argument("--stream-ordered", type=int, default=0, choices=[0, 1],
                    help="opts_init.stream_ordered: with device arrays step_sync returns once its work is queued on the object's stream "
                         "(the host queues step_async while condensation runs) instead of waiting for th and rv as the reference's does")
    ap.add_argument("--reorder-every", type=int, default=0,
                    help="opts_init.reorder_every: physical re-ordering of the super-droplet storage into the cell order every so "
                         "many steps (0 = the library default, every 64 steps -- 32 for slabs with neighbours -- and with every compaction; -1 = never, the reference's "
                         "storage order)")
    ap.add_argument("--workload", choices=["stratocumulus", "coal-stress"], default="stratocumulus",
                    help="stratocumulus (default): BASELINE configs[2], activating aerosol, few collisions; coal-stress: SURVEY 8(d) C5 variant "
                         "(ii), the Golovin test's drizzle spectrum under hall_davis_no_waals -- a per cent of the candidate pairs collide "
                         "per second; the result line then carries `coal_stress` (collided pairs per step, k_coal's rate with its write-back)")
    ap.add_argument("--kernel", default=None, help="collision kernel by its name in lgrngn.kernel_t (default: the workload's)")
    ap.add_argument("--dt", type=float, default=1., help="time step in seconds")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-leg", action="store_true",
                    help="skip the short measurement with the Eulerian arrays in HOST memory (numpy arrays through arrinfo_t, what an "
                         "unchanged icicle / UWLCM passes), reported as `host_arrays` next to the headline figure")
    ap.add_argument("--no-toms-leg", action="store_true",
                    help="skip the short measurement with opts_init.cond_solver = 1 (the reference's TOMS748 iterates in fast arithmetic), "
                         "reported as `cond_solver_toms748` next to the headline figure")
    ap.add_argument("--leg-steps", type=int, default=20, help="steps of the host-array and cond_solver legs")
    ap.add_argument("--no-strict-leg", action="store_true",
                    help="skip the second, short measurement with opts_init.strict_fp = 1 (the API's default arithmetic: IEEE operation "
                         "order, what a caller who changes nothing gets), reported as `strict_fp` next to the headline figure")
    ap.add_argument("--strict-leg-steps", type=int, default=20)
    ap.add_argument("--cpu-sample-n", type=int, default=128)
    ap.add_argument("--cpu-sample-steps", type=int, default=2)
    ap.add_argument("--no-stage-timers", action="store_true", help="no hipEvents at all (neither the condensation stage's in the timed region nor the stage pass)")
    ap.add_argument("--stage-steps", type=int, default=20, help="extra steps behind the timed region with every stage's hipEvents on: the stage table (0: none)")
    ap.add_argument("--oversubscribe", action="store_true", help="--gpus N in one process with all N slabs on device 0")
    ap.add_argument("--spmd", action="store_true", help="(the default under torch.distributed.run; kept for older command lines)")
    ap.add_argument("--native", action="store_true",
                    help="under torch.distributed.run: rank 0 drives all N devices with the native multi_HIP object (one host thread per "
                         "device, migrants written into the neighbour's memory), the other ranks only join the barriers; default "
                         "there: one single-device object per rank with the migrants over RCCL (libcloudphxx_amd.multi)")
    ap.add_argument("--self-ring", action="store_true",
                    help="ONE rank of the one-object-per-rank path whose neighbours on both sides are the rank itself: its migrants leave "
                         "and arrive through RCCL -- what a one-GPU box can measure of that path (with --nx: one slab of an N-way split, "
                         "its exchange included).  The droplets are those of the periodic box; only their route differs.")
    ap.add_argument("--transport", choices=["rccl", "host"], default=None,
                    help="one object per rank: how the migrants travel -- device buffers over RCCL (default with one GPU per rank), or "
                         "staged through the host over gloo (default when the ranks share a GPU)")
    ap.add_argument("--processes", default="all", choices=["cond", "cond+coal", "cond+coal+adve", "all"],
                    help="which processes a step runs (opts_t.cond / coal / adve / sedi), as the reference's timing sweep does "
                         "(models/kinematic_2D/tests/paper_GMD_2015/fig_b/calc.cpp:49: a / ac / acc / accs): substeps timed in isolation; "
                         "the headline and every leg of the default line run all of them")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip the coal_stress, c5, c2, soak and activation legs of the default line")
    ap.add_argument("--soak-steps", type=int, default=1000, help="steps of the default line's soak leg (the headline's configuration, long window)")
    ap.add_argument("--dbg", default="",
                    help="comma-separated names of opts_init.dbg_flags bits (libcloudphxx_amd.lgrngn.dbg: test / measurement switches, "
                         "e.g. NO_DEFERRED_SORT,COND_SORTED_ORDER,MULTI_SERIALIZE); the library reads no such switch from the environment")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: the condensation stage's events in the timed region, the stage pass, the roofline "
                         "and the device's copy bandwidth, the coal-stress figures, the legs and the CPU baseline.  Without it a run sets up, "
                         "warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the caller holds after the last one -- th and rv, which step_sync updates in "
                         "place -- as DIR/th.npy and DIR/rv.npy (see dump_outputs)")
    args = ap.parse_args()

    # stdout carries ONE line, the result.  Libraries that write to file descriptor 1 on their own (RCCL prints a version banner from
    # C stdio when its first communicator comes up, flushed at exit, i.e. AFTER the result) go to stderr instead.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))          # > 1: launched by torch.distributed.run, one process per GPU
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and world != args.gpus:
        raise SystemExit("--gpus %d does not match the launcher's WORLD_SIZE %d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP backend has no CPU fallback)")
    # As ONE process, --gpus N > 1 runs the library's native multi_HIP object (one host thread per device, migrants written straight
    # into the neighbour's memory over xGMI).  Under torch.distributed.run (WORLD_SIZE = N) every rank owns one slab on its own GPU
    # and the migrants travel over RCCL (libcloudphxx_amd.multi) -- the launcher's N processes are N working ranks; --native lets
    # rank 0 drive all N devices with the native object instead (the other ranks then only join the barriers).
    if args.self_ring and (world > 1 or args.gpus > 1):
        raise SystemExit("--self-ring is the one-rank form of the one-object-per-rank path: no launcher, --gpus 1")
    spmd = (world > 1 and not args.native) or args.self_ring
    if args.dump_outputs and spmd and world > 1:
        raise SystemExit("--dump-outputs needs the whole box in one process: --gpus N without a launcher, or --native under one")
    stage_timers = args.full and not args.no_stage_timers
    native_multi = args.gpus > 1 and not spmd
    idle = native_multi and rank > 0
    n_slabs = args.gpus
    if native_multi and not idle:
        if args.oversubscribe:
            os.environ["LCX_MULTI_DEVICE_MAP"] = ",".join(["0"] * args.gpus)
        dmap = os.environ.get("LCX_MULTI_DEVICE_MAP")
        slab_dev = [int(x) for x in dmap.split(",")][:args.gpus] if dmap else list(range(args.gpus))
        if max(slab_dev) >= torch.cuda.device_count() and world == 1:      # (under a launcher: the per-rank fallback below)
            raise SystemExit("--gpus %d: only %d device(s) visible (use --oversubscribe to put every slab on device 0)"
                             % (args.gpus, torch.cuda.device_count()))
    dev_index = local_rank % torch.cuda.device_count() if spmd else 0
    if not idle:
        torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    import torch.distributed as dist
    if world > 1:
        import datetime
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # host-side collectives (barriers, the timing reduction) over gloo, so that a waiting rank sleeps on the host instead of
        # spinning in a kernel on a GPU that rank 0 is driving; device tensors (the SPMD path's migrants) go over RCCL
        dist.init_process_group("cpu:gloo,cuda:nccl", timeout=datetime.timedelta(minutes=60))
    elif args.self_ring:
        import socket
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        dist.init_process_group("cpu:gloo,cuda:nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)

    from libcloudphxx_amd import lgrngn, multi
    real_t = np.float64 if args.real == "f64" else np.float32
    tdtype = torch.float64 if args.real == "f64" else torch.float32
    n = args.n
    nx_tot = n * n_slabs if args.scaling == "weak" else n
    if args.nx:
        nx_tot = args.nx
    ny, nz = args.ny or n, args.nz or n
    oi = make_opts_init(nx_tot, ny, nz, args.sd_conc, args.dx, args.sstp_cond, args.sstp_coal, 44 + rank, args.workload, args.dt, args.kernel)
    oi.dev_id = -1 if native_multi else dev_index
    oi.strict_fp = args.strict_fp
    oi.cond_solver = 1 if args.cond_solver == "toms748" else 0
    oi.reorder_every = args.reorder_every
    oi.stream_ordered = bool(args.stream_ordered)
    for name in filter(None, args.dbg.split(",")):
        if name.strip().startswith("budget="):
            oi.dbg_cond_budget = int(name.split("=")[1])
        else:
            oi.dbg_flags |= int(lgrngn.dbg[name.strip()])
    if args.cond_mode != "percell":
        oi.exact_sstp_cond = True
        oi.sstp_cond_mix = args.cond_mode == "pp_mix"
        oi.adaptive_sstp_cond = args.cond_mode == "pp_adaptive"
        oi.n_sd_max = int(oi.n_sd_max)

    def device_fields(nx_loc, x_off, d):
        class TorchXP:                      # the tiny subset of the numpy namespace make_fields uses, on the device
            @staticmethod
            def arange(m, dtype=None):
                return torch.arange(m, dtype=tdtype, device=d)
            sin, cos, exp, log = staticmethod(torch.sin), staticmethod(torch.cos), staticmethod(torch.exp), staticmethod(torch.log)
        f = make_fields(nx_loc, ny, nz, x_off, nx_tot, TorchXP, tdtype)
        shapes = [(nx_loc, ny, nz)] * 3 + [(nx_loc + 1, ny, nz), (nx_loc, ny + 1, nz), (nx_loc, ny, nz + 1)]
        return [t.expand(sh).contiguous() for t, sh in zip(f, shapes)]

    n_sd_max0 = oi.n_sd_max

    def setup_native():
        """ONE object over args.gpus devices; the Eulerian arrays live in per-slab pieces on the slabs' own devices"""
        oi.dev_count, oi.dev_id = args.gpus, -1
        oi.n_sd_max = int(n_sd_max0 * 1.1)              # (per slab: n_sd_max / dev_count + 1, distmem_opts.hpp:47)
        prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi, real_t)
        per = nx_tot // args.gpus
        parts = [device_fields(per if r < args.gpus - 1 else nx_tot - r * per, r * per, torch.device("cuda", slab_dev[r]))
                 for r in range(args.gpus)]
        arrays = [lgrngn.DeviceArrays([parts[r][k].data_ptr() for r in range(args.gpus)], parts[0][k].shape) for k in range(6)]
        return prt, parts, arrays, sorted(set(slab_dev))

    probe_state = {"hung": False}

    def rccl_ring_works():
        """one small message to either neighbour and back, the way libcloudphxx_amd/multi.py posts them (a batch of isend / irecv on
        device tensors); every rank learns whether EVERY rank got through -- a node whose RCCL cannot do that still gets measured"""
        # The probe runs in a thread of its own with a deadline: a point-to-point operation that HANGS (instead of raising) must not hold
        # every rank until the process group's time-out.  A probe that has not come back after 90 s counts as failed; its thread is left
        # behind (it sits in a blocking wait that nothing can cancel), the run goes on over the host transport, and the process ends
        # with os._exit so that the abandoned communicator cannot block the interpreter's shutdown.
        import threading
        res = {"ok": 0, "err": None}

        def probe():
            try:
                torch.cuda.set_device(dev)
                lft, rgt = (rank - 1) % world, (rank + 1) % world
                out_l = torch.full((256,), float(rank), device=dev); out_r = out_l.clone()
                in_l = torch.empty(256, device=dev); in_r = torch.empty(256, device=dev)
                ops = [dist.P2POp(dist.isend, out_l, lft), dist.P2POp(dist.isend, out_r, rgt),
                       dist.P2POp(dist.irecv, in_r, rgt), dist.P2POp(dist.irecv, in_l, lft)]
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
                torch.cuda.synchronize(dev)
                res["ok"] = int(float(in_l[0]) == float(lft) and float(in_r[0]) == float(rgt))
            except Exception as e:                           # (RuntimeError / DistBackendError: no link, no IPC, ...)
                res["err"] = str(e)
        th_ = threading.Thread(target=probe, daemon=True)
        th_.start()
        th_.join(90.)
        ok = res["ok"]
        if th_.is_alive():
            ok = 0
            probe_state["hung"] = True
            print("bench.py rank %d: the RCCL ring probe did not return within 90 s" % rank, file=sys.stderr, flush=True)
        elif res["err"]:
            print("bench.py rank %d: RCCL ring probe: %s" % (rank, res["err"]), file=sys.stderr, flush=True)
        t = torch.tensor([ok])
        dist.all_reduce(t, op=dist.ReduceOp.MIN)             # (gloo)
        return bool(int(t.item()))

    def setup_local():
        """a single-device object: the whole domain, or this rank's slab of the one-object-per-rank run"""
        oi.dev_count, oi.dev_id, oi.n_sd_max = 0, dev_index, n_sd_max0
        if spmd:
            shared_gpu = torch.cuda.device_count() < world           # several ranks on one device: RCCL refuses that, stage through the host
            transport = args.transport or ("host" if shared_gpu else "rccl")
            if transport == "rccl" and world > 1 and not rccl_ring_works():
                transport = "host"
                if rank == 0:
                    print("bench.py: a device-to-device ring exchange over RCCL failed on this node; the migrants are staged through the host",
                          file=sys.stderr, flush=True)
            prt = multi.particles_multi_t(oi, real_t, device=dev, transport=transport, self_ring=args.self_ring)
            nx_loc, x_off = prt.opts_init.nx, prt.n_x_bfr
        else:
            prt = lgrngn.factory(lgrngn.backend_t.HIP, oi, real_t)
            nx_loc, x_off = nx_tot, 0
        fields = device_fields(nx_loc, x_off, dev)
        return prt, fields, [lgrngn.DeviceArray(t.data_ptr(), t.shape) for t in fields], [dev_index]

    def setup_and_init(setup):
        prt, keep, arrays, devices = setup()
        for d in devices:
            torch.cuda.synchronize(d)
        t0 = time.perf_counter()
        prt.init(arrays[0], arrays[1], arrays[2], Cx=arrays[3], Cy=arrays[4], Cz=arrays[5])
        for d in devices:
            torch.cuda.synchronize(d)
        return prt, keep, arrays, devices, time.perf_counter() - t0

    state, fallback_reason = None, None
    if (native_multi and not idle and len(set(slab_dev)) > 1) or world > 1:
        # several real devices (in one process, or one rank each), never run on this hardware before this bench: a cross-device wait
        # or a point-to-point operation that never returns must not hold the launcher for its whole time-out -- give up loudly after
        # 30 minutes (a default run takes about one)
        import threading

        def _give_up():
            print("bench.py: the multi-device run did not finish within 1800 s; giving up", file=sys.stderr, flush=True)
            os._exit(3)
        _watchdog = threading.Timer(1800., _give_up)
        _watchdog.daemon = True
        _watchdog.start()
    if native_multi:
        if not idle:
            try:
                if max(slab_dev) >= torch.cuda.device_count():
                    raise RuntimeError("slab devices %s: only %d device(s) visible" % (slab_dev, torch.cuda.device_count()))
                state = setup_and_init(setup_native)
            except RuntimeError as e:
                if world == 1:
                    raise
                fallback_reason = str(e)
        if world > 1:                                   # every rank learns whether rank 0 got its multi-device object
            ok = torch.tensor([0 if fallback_reason else 1])
            dist.broadcast(ok, 0)
            if not int(ok.item()):
                if rank == 0:
                    print("bench.py: native multi_HIP object failed (%s); falling back to one object per rank over RCCL"
                          % fallback_reason, file=sys.stderr, flush=True)
                spmd, native_multi, idle, state = True, False, False, None
                dev_index = local_rank % torch.cuda.device_count()
                torch.cuda.set_device(dev_index)
                dev = torch.device("cuda", dev_index)
    if state is None and not idle:
        state = setup_and_init(setup_local)
    if idle:
        prt, fields_t, devices, t_init = None, None, [], 0.
        th = rv = rhod = Cx = Cy = Cz = None
    else:
        prt, fields_t, (th, rv, rhod, Cx, Cy, Cz), devices, t_init = state

    def sync_all():
        for d in devices:
            torch.cuda.synchronize(d)
    opts = lgrngn.opts_t()
    opts.cond = True
    opts.coal = args.processes in ("cond+coal", "cond+coal+adve", "all")
    opts.adve = args.processes in ("cond+coal+adve", "all")
    opts.sedi = args.processes == "all"

    def barrier():
        sync_all()
        if world > 1:
            dist.all_reduce(torch.zeros(1))             # (gloo: a host barrier)
        sync_all()

    def one_step():
        prt.step_sync(opts, th, rv, rhod, Cx, Cy, Cz)
        prt.step_async(opts)

    sd_done = 0
    if idle:                                            # rank 0 drives this rank's device: only the barriers and the reduction
        barrier()
        t0 = time.perf_counter()
        barrier()
        elapsed = time.perf_counter() - t0
        stage_ms = {}
    else:
        for _ in range(args.warmup):
            one_step()
        p1 = prt.prt if spmd else prt
        # the timed region carries the events of the dominant kernel's stage only (the roofline's launch duration, two records per
        # step); the stage table comes from a few EXTRA steps with every stage's events on -- each record is a packet between two kernels,
        # and fifty of them per step cost a 16-plane slab 0.11 ms of its 1.33 ms step (0.04 of C3's 10).  Both only with --full.
        if stage_timers:
            p1.set_profiling(2)
        barrier()
        n_part_start = p1.n_part
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_step()
            sd_done += p1.n_part
        barrier()
        elapsed = time.perf_counter() - t0
        n_part_end = p1.n_part
        if args.dump_outputs:
            if spmd and world > 1:                           # (the native object failed under a launcher: every rank holds a slab)
                raise SystemExit("--dump-outputs: the native multi_HIP object failed, every rank holds only its own slab")
            slabs = fields_t if native_multi else [fields_t]      # (native multi_HIP: th and rv in per-slab pieces, joined along x)
            dump_outputs(args.dump_outputs, {nm: np.concatenate([s[k].cpu().numpy() for s in slabs]) for k, nm in ((0, "th"), (1, "rv"))})
        tm_ = p1.timings() if stage_timers else {}
        cond_ms = tm_.get("cond")
        listed_ms_total = tm_.get("cond_listed")
        stage_ms = {}
        if stage_timers and args.stage_steps > 0:
            p1.set_profiling(1)
            for _ in range(args.stage_steps):
                one_step()
            sync_all()                                       # (no rendezvous with the other ranks: they are in the same loop, or idle)
            stage_ms = {k: (v * args.steps / args.stage_steps if k != "rendezvous_hidden_share" else v) for k, v in p1.timings().items()}
        if stage_timers:
            p1.set_profiling(0)
        if cond_ms is not None:
            stage_ms["cond"] = cond_ms                       # (the timed region's own)
            if listed_ms_total is not None:
                stage_ms["cond_listed"] = listed_ms_total
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = torch.tensor([float(sd_done)], dtype=torch.float64)
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        elapsed, sd_total = float(tmax[0]), float(tsum[0])
    else:
        sd_total = float(sd_done)
    world_out = n_slabs if (native_multi or spmd) else 1

    if rank == 0:
        R = 8 if args.real == "f64" else 4
        # ALGORITHMIC bytes of the dominant kernel (k_cond), SURVEY 8(d): 5R (rw2,rd3,kpa,vt read + rw2 write)
        # + I (sorted_id + sorted_ijk, two u32 = 8 B) + N (multiplicity, 8 B) per super-droplet per substep
        cond_bytes_per_sd = 5 * R + 8 + 8
        n_local = sd_done / max(args.steps, 1) / (n_slabs if native_multi else 1)      # super-droplets per device and step
        roof = None
        if "cond" in stage_ms and args.cond_mode == "percell":
            launches = args.steps * args.sstp_cond
            avg_ms = stage_ms["cond"] / launches
            ach = cond_bytes_per_sd * n_local / (avg_ms * 1e-3) / 1e9
            kname = "k_cond" if args.strict_fp else "k_cond_lean" if args.cond_solver == "lean" else "k_cond_lean<.., SOLVER = TOMS748>"
            roof = {"bound": "hbm", "kernel": kname, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": ach / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": avg_ms,
                    "algorithmic_bytes_per_sd": cond_bytes_per_sd, "algorithmic_bytes": cond_bytes_per_sd * n_local}
            # On a single device the storage-order kernel also does the SCATTER of the previous step's re-sort (k_scatter_sorted's loads
            # and stores, 3I + 2I = 20 B per SD: cell index and arrival rank read, cell offset gathered, sorted id and sorted cell written)
            # in every step but the storage re-ordering ones.  `achieved` / `frac` stay on the condensation's own 56 B;
            # the launch's whole algorithmic traffic is given beside them.
            if (not args.strict_fp and args.cond_solver == "lean" and world_out == 1 and not args.self_ring and args.sstp_cond == 1
                    and not oi.dbg_flags & int(lgrngn.dbg.NO_DEFERRED_SORT | lgrngn.dbg.COND_SORTED_ORDER)):
                carried = 5 * 4
                roof["carries"] = "the scatter of the previous step's re-sort (k_scatter_sorted: %d B per SD), except in storage re-ordering steps" % carried
                roof["achieved_with_carried"] = (cond_bytes_per_sd + carried) * n_local / (avg_ms * 1e-3) / 1e9
                roof["frac_with_carried"] = roof["achieved_with_carried"] / HBM_PEAK_GBS
            if not args.strict_fp and args.cond_solver == "lean" and world_out == 1 and not args.self_ring:
                # (late round 5) the stage's time includes k_cond_lean_listed: the droplets whose bracket can hold several roots, solved
                # with the reference's TOMS748 iterates -- how many of them the last step had
                try:
                    roof["listed_for_the_references_iterates"] = int(p1.state_u64("raw_cond_listed")[0])
                    roof["listed_share"] = roof["listed_for_the_references_iterates"] / max(n_local, 1.)
                except Exception:
                    pass
                # (round 6) `avg_launch_ms` is k_cond_lean's launch alone; the listed droplets' kernel (k_cond_lean_listed, beside the in-cell
                # ranking in the timed region) is a stage of its own
                if "cond_listed" in stage_ms:
                    roof["listed_ms"] = stage_ms["cond_listed"] / launches
            # HBM bytes and instruction counts per launch from the PMC passes of tools/profile_round.sh (FETCH_SIZE x 2 + WRITE_SIZE,
            # KiB; counters cannot be collected inside a timed run): reported only for the configuration they were measured on
            default_cfg = (world_out == 1 and n == 128 and not (args.nx or args.ny or args.nz) and args.sd_conc == 64 and args.real == "f64"
                           and not args.strict_fp and args.sstp_cond == 1 and args.cond_solver == "lean")
            if default_cfg:
                import glob
                for tf in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))[-1:]:
                    tj = json.load(open(tf))
                    both = [v for k_, v in tj.items() if k_.startswith("lcx::k_cond_lean<double")]
                    t = {k_: sum(v.get(k_, 0) for v in both) for k_ in set().union(*both) if isinstance(both[0].get(k_, 0), (int, float))} if both else None
                    if t:
                        src = "profiles/" + os.path.basename(tf)
                        roof["traffic"] = t["hbm_bytes"]
                        roof["traffic_source"] = src
                        roof["traffic_launches"] = (tj.get("_meta") or {}).get("launches", "launches 2-3 of a fresh box (a profile of rounds 1-5)")
                        # what the launch MOVES per super-droplet by the counters (the run's single hygroscopicity is a scalar: 8 of the
                        # 56 algorithmic bytes are not read) -- `frac_with_carried` prices 76 algorithmic bytes, not these
                        roof["bytes_moved_per_sd"] = t["hbm_bytes"] / n_local
                        roof["achieved_on_bytes_moved"] = t["hbm_bytes"] / (avg_ms * 1e-3) / 1e9
                        roof["frac_on_bytes_moved"] = roof["achieved_on_bytes_moved"] / HBM_PEAK_GBS
                        if "hbm_bytes_low" in t:
                            # FETCH_SIZE counts requests, not bytes: 128-B requests (coalesced reads) and 64-B ones (sparse gathers) look
                            # alike.  `traffic` prices every read request at 128 B (an upper bound), `traffic_low` at 64 B (a lower one);
                            # calibration: profiles/r03_traffic_calibration.json
                            roof["traffic_low"] = t["hbm_bytes_low"]
                        if "valu_insts" in t:
                            # the second roof: fp64 vector arithmetic.  78.6 TFLOP/s = 256 CUs x 4 SIMDs x 16 fp64 FMA lanes x 2 x 2.4 GHz.
                            # lane_util = share of the 64 lanes that were active per VALU instruction
                            f64 = t.get("valu_f64_insts", 0)
                            flop = (2 * t.get("valu_fma_f64", 0) + t.get("valu_mul_f64", 0) + t.get("valu_add_f64", 0) + t.get("valu_trans_f64", 0)) * 64
                            lane = t["thread_cycles_valu"] / (t["valu_insts"] * 64) if t.get("thread_cycles_valu") else None
                            roof["fp64_valu"] = {"achieved_tflops": flop / (avg_ms * 1e-3) / 1e12, "peak_tflops": 78.6,
                                                 "frac": flop / (avg_ms * 1e-3) / 1e12 / 78.6,
                                                 "useful_tflops": (flop * lane / (avg_ms * 1e-3) / 1e12) if lane else None,
                                                 # share of the cycles in which the vector ALUs executed, from the counters of the same PMC
                                                 # passes: SQ_ACTIVE_INST_VALU (quad-cycles) x 4 / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs)
                                                 "issue_frac": (t["active_inst_valu"] * 4 / (1024 * t["grbm_gui_active"] / 8)
                                                                if t.get("active_inst_valu") and t.get("grbm_gui_active") else None),
                                                 "lane_util": lane,
                                                 "wave_insts_per_launch": t["valu_insts"], "f64_insts_per_launch": f64, "source": src}
        # attainable HBM bandwidth on this device (device-to-device copy of 1 GiB, read + write), SURVEY 8(d)
        copy_gbs = None
        if args.full:
            a_ = torch.empty(1 << 30, dtype=torch.uint8, device=dev); b_ = torch.empty_like(a_)
            b_.copy_(a_); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                b_.copy_(a_)
            e1.record(); torch.cuda.synchronize()
            copy_gbs = 10 * 2 * a_.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e9
            del a_, b_
        # per-stage achieved algorithmic bandwidth (bytes per SD from SURVEY 8(d) with 4-byte indices: I = 4)
        I = 4
        stage_bytes = {"cond": 5 * R + 2 * I + 8, "cond_cellfinish": (1 if not args.strict_fp else 2) * R, "hskpng_vterm_all": 2 * R + I,
                       "hskpng_shuffle_and_sort": 2 * I, "coal": 2 * I + R / 2 + 8 + 3 * R,
                       "move(adve+sedi+bcnd)": 7 * R + 2 * I, "post_copy": 3 * I}
        # the in-cell shuffle of coalescence is done by the re-sort at the end of the previous step in production order: one entry
        sort_ms = stage_ms.get("post_copy", 0.) + stage_ms.get("hskpng_shuffle_and_sort", 0.)
        stage_bytes["re-sort (post_copy + in-cell shuffle)"] = stage_bytes.pop("post_copy") + stage_bytes.pop("hskpng_shuffle_and_sort")
        stage_ms_r = dict(stage_ms)
        stage_ms_r["re-sort (post_copy + in-cell shuffle)"] = sort_ms
        stage_roof = {}
        coal_stress = None
        if args.full and args.workload == "coal-stress" and world_out == 1 and not args.self_ring:
            # pairs that collided in the last step: the living super-droplets that carry coalescence's invalid terminal velocity
            # (the one of each pair that grew); a collided pair writes back N + 3R bytes (n of the one, rw2, rd3, vt of the other)
            pairs = int(p1.state_u64("raw_collided")[0])
            wb = (8 + 3 * R) * pairs / max(n_local, 1.)
            stage_bytes["coal"] += wb
            coal_stress = {"collided_pairs_per_step": pairs, "share_of_candidate_pairs": pairs / max(n_local / 2., 1.),
                           "write_back_bytes_per_sd": wb, "super_droplets_lost_per_step": (n_part_start - n_part_end) / max(args.steps, 1),
                           "spectrum": "n(ln r) = 3 n0 (r/r0)^3 exp(-(r/r0)^3), r0 = 30.084 um, n0 = 2^23 m^-3, kappa = 1e-10 "
                                       "(ref tests/python/physics/coalescence_golovin.py:31-44)"}
        for k_, bsd in stage_bytes.items():
            if k_ in stage_ms_r and stage_ms_r[k_] > 0:
                gbs = bsd * n_local / (stage_ms_r[k_] / args.steps * 1e-3) / 1e9
                stage_roof[k_] = {"bytes_per_sd": bsd, "GB/s": gbs, "frac_of_8TB/s": gbs / HBM_PEAK_GBS}
        if roof is not None:
            roof["peak_measured_copy_GBs"] = copy_gbs
        if native_multi:
            decomposition_note = " (native multi_HIP object: one process, one host thread per device, migrants written into the neighbour's memory%s%s)" % (
                "; all slabs on device 0" if args.oversubscribe else "",
                "; driven by rank 0 of the launcher, ranks 1..%d idle" % (world - 1) if world > 1 else "")
        elif spmd:
            decomposition_note = " (%s, migrants %s, %d second-part exchanges on rank 0%s)" % (
                "ONE rank whose neighbours are the rank itself (--self-ring)" if args.self_ring else "one single-device object per rank",
                "over RCCL" if prt.transport == "rccl" else "staged through the host over gloo (ranks share a GPU)", prt.second_rounds,
                "; fallback: " + fallback_reason if fallback_reason else "")
        else:
            decomposition_note = ""
        prt_transport = getattr(prt, "transport", None) if spmd else None
        prt_second_rounds = getattr(prt, "second_rounds", None) if spmd else None
        out = {
            "metric": "super-droplets/sec (cond+coal substep), 128^3 x 64 SD/cell",
            "value": sd_total / elapsed,
            "unit": "super-droplets/s",
            "n_gpus": world_out, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": args.real,
            "data": "synthetic",
            "config": {"workload": "3-D box %dx%dx%d cells x %d SD/cell, %s, sstp %d/%d, kernel %s, vt beard77fast"
                                   % (nx_tot, ny, nz, args.sd_conc, "cond+coal+adve+sedi+bcnd" if args.processes == "all" else args.processes + " only",
                                      args.sstp_cond, args.sstp_coal, lgrngn.kernel_t(oi.kernel).name),
                       "super_droplets": int(sd_total / args.steps), "decomposition": "x-slabs:%d%s" % (world_out, decomposition_note), "cond_mode": args.cond_mode,
                       "fp_mode": "strict IEEE order, TOMS748 iterates" if args.strict_fp else
                                  "fp64, growth rate as one rational expression + FMA; " + ("lean bracketed secant to the reference's tolerance 2^-15" if args.cond_solver == "lean"
                                                                                             else "the reference's TOMS748 iterates"),
                       "init_s": t_init},
        }
        if args.full:
            out.update({
                "roofline": roof,
                # `cond` from the timed region; the other stages from args.stage_steps extra steps (scaled to the same per-step unit)
                "stage_ms_per_step": {k: (v / args.steps if k != "rendezvous_hidden_share" else v) for k, v in stage_ms.items()},
                "stage_pass_steps": args.stage_steps if stage_timers else 0,
                # (the stage pass times the stages ONE AFTER THE OTHER.  In the timed region the in-cell ranking -- most of post_copy -- runs on
                # a stream of its own next to cond_cellfinish, sync_out, hskpng_Tpr and hskpng_vterm_all, so the stages add up to more than
                # ms_per_step)
                "stage_note": "stages timed serially by the stage pass; in the timed region post_copy's in-cell ranking overlaps cond_cellfinish .. hskpng_vterm_all",
                "stage_roofline": stage_roof,
            })
        if spmd or native_multi:
            # what ran, for a reader of an N-GPU record: how many ranks did work, how the migrants travelled, how often a message needed
            # its second part
            out["config"]["ranks_working"] = 1 if (native_multi and world > 1) else world_out
            out["config"]["transport"] = ("peer writes / peer copies inside one process (native multi_HIP object)" if native_multi
                                          else prt_transport)
            out["config"]["second_rounds"] = None if native_multi else prt_second_rounds
        if coal_stress is not None:
            coal_stress["coal_ms"] = out["stage_ms_per_step"].get("coal")
            coal_stress["reorder_storage_ms"] = out["stage_ms_per_step"].get("reorder_storage")
            coal_stress["post_copy_ms"] = out["stage_ms_per_step"].get("post_copy")
            out["coal_stress"] = coal_stress
        legs_ok = args.full and world_out == 1 and args.cond_mode == "percell" and not args.self_ring
        if legs_ok:
            # Further SHORT measurements on the same box, each on an object of its own built from the headline's options with one thing
            # changed.  The headline object goes first (its two attribute sets and housekeeping are tens of GB), and every leg gets
            # fresh input fields (the headline run has evolved th and rv in place).
            import gc
            prt = p1 = state = fields_t = None
            th = rv = rhod = Cx = Cy = Cz = None
            gc.collect()
            torch.cuda.synchronize()

            def run_leg(change, steps, host_arrays=False, collisions=False, forcing=None, listed=False):
                """host_arrays: False (device arrays), True (all six as host arrays in every step: UWLCM's call), "thrv" (host arrays, th and
                rv only in every step: icicle's call, kin_cloud_2d_lgrngn.hpp:242-246); forcing(it, tensors): the caller's own change of
                its device arrays between two steps; listed: the share of droplets that the condensation kernel lists, sampled"""
                keep = {k: getattr(oi, k) for k in change}
                for k, v in change.items():
                    setattr(oi, k, v)
                try:
                    f = device_fields(nx_tot, 0, dev)
                    arrs = [t.cpu().numpy() for t in f] if host_arrays else [lgrngn.DeviceArray(t.data_ptr(), t.shape) for t in f]
                    pr = lgrngn.factory(lgrngn.backend_t.HIP, oi, real_t)
                    pr.init(arrs[0], arrs[1], arrs[2], Cx=arrs[3], Cy=arrs[4], Cz=arrs[5])
                    if host_arrays == "thrv":
                        arrs = arrs[:2]
                    it_ = [0]

                    def force():
                        if forcing is not None:
                            forcing(it_[0], f)
                            torch.cuda.synchronize()
                        it_[0] += 1
                    for _ in range(3):
                        force()
                        pr.step_sync(opts, *arrs)
                        pr.step_async(opts)
                    # timed as the headline is: the condensation stage's two events per step and nothing else (level 2); the stage table
                    # from a few extra steps with every stage's events on (level 1: the stages then run one after the other)
                    pr.set_profiling(2)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    done = 0
                    for _ in range(steps):
                        force()
                        pr.step_sync(opts, *arrs)
                        pr.step_async(opts)
                        done += pr.n_part
                    torch.cuda.synchronize()
                    dt_ = time.perf_counter() - t0
                    tm2_ = pr.timings()
                    cond_ms_ = tm2_.get("cond", 0.) / max(steps * args.sstp_cond, 1)
                    listed_ms_ = tm2_.get("cond_listed", 0.) / max(steps * args.sstp_cond, 1)
                    listed_share_ = None
                    if listed:
                        # (sampled behind the timed loop, a read-back per step: 16 more steps -- one period of the activation leg's forcing)
                        sh_ = []
                        for _ in range(16):
                            force()
                            pr.step_sync(opts, *arrs)
                            sh_.append(int(pr.state_u64("raw_cond_listed")[0]) / max(pr.n_part, 1))
                            pr.step_async(opts)
                        listed_share_ = {"mean": float(np.mean(sh_)), "max": float(np.max(sh_)), "min": float(np.min(sh_))}
                    stage_steps_ = min(4, steps)
                    pr.set_profiling(1)
                    for _ in range(stage_steps_):
                        force()
                        pr.step_sync(opts, *arrs)
                        pr.step_async(opts)
                    torch.cuda.synchronize()
                    st_ = pr.timings()
                    ach_ = cond_bytes_per_sd * (done / steps) / (cond_ms_ * 1e-3) / 1e9 if cond_ms_ else None
                    n_end = pr.n_part
                    pairs_ = int(pr.state_u64("raw_collided")[0]) if collisions else None
                    res = {"value": done / dt_, "unit": "super-droplets/s", "ms_per_step": dt_ / steps * 1e3, "steps": steps,
                           "roofline": {"bound": "hbm", "achieved": ach_, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                        "frac": ach_ / HBM_PEAK_GBS if ach_ else None, "avg_launch_ms": cond_ms_,
                                        "algorithmic_bytes_per_sd": cond_bytes_per_sd},
                           "stage_ms_per_step": {k: v / stage_steps_ for k, v in st_.items()}}
                    if listed:
                        res["cond_ms"] = cond_ms_
                        res["listed_ms"] = listed_ms_
                        res["listed_share"] = listed_share_
                    if collisions:
                        # pairs that collided in the last step (the living super-droplets that carry coalescence's invalid terminal velocity);
                        # a collided pair writes back N + 3R bytes (n of the one, rw2, rd3, vt of the other)
                        n_sd_ = done / steps
                        res["collided_pairs_per_step"] = pairs_
                        res["share_of_candidate_pairs"] = pairs_ / max(n_sd_ / 2., 1.)
                        res["coal_ms"] = res["stage_ms_per_step"].get("coal")
                        res["coal_bytes_per_sd"] = stage_bytes["coal"] + (8 + 3 * R) * pairs_ / max(n_sd_, 1.)
                        res["coal_GBs"] = (res["coal_bytes_per_sd"] * n_sd_ / (res["coal_ms"] * 1e-3) / 1e9) if res["coal_ms"] else None
                        res["cond_ms"] = cond_ms_
                        res["super_droplets"] = int(n_sd_)
                    del pr, f, arrs
                    gc.collect()
                    torch.cuda.synchronize()
                    return res
                finally:
                    for k, v in keep.items():
                        setattr(oi, k, v)

            if not args.strict_fp and args.cond_solver == "lean" and not args.no_toms_leg:
                # THE API DEFAULT since round 5 (both host mirrors, lcx_opts_init_default): fast arithmetic with the reference's TOMS748
                # iterates (the reference's answer is the midpoint of ITS last bracket) -- held to SURVEY 8a's bars in every test, where
                # the headline's lean solver is held to its own (tests/_harness.py).  What a driver that changes no option gets.
                out["api_default"] = run_leg({"strict_fp": False, "cond_solver": 1}, args.leg_steps)
                out["api_default"]["fp_mode"] = "fast arithmetic, the reference's TOMS748 iterates (opts_init.strict_fp = 0, cond_solver = 1: the API default)"
                out["api_default"]["roofline"]["kernel"] = "k_cond_lean<.., SOLVER = TOMS748>"
            if not args.no_host_leg:
                # what an unchanged icicle / UWLCM gets: the Eulerian arrays in HOST memory (numpy arrays through arrinfo_t) -- sync_in /
                # sync_out include the PCIe transfers and the host-side row copies.  Once with every option as in the headline, once with
                # the API's default arithmetic: the caller that changes nothing at all
                arrays_note = "th, rv, rhod, Cx, Cy, Cz as host (numpy) arrays: %.1f MB in, %.1f MB out per step" % (
                    (3 * nx_tot * ny * nz + (nx_tot + 1) * ny * nz + nx_tot * (ny + 1) * nz + nx_tot * ny * (nz + 1)) * R / 1e6, 2 * nx_tot * ny * nz * R / 1e6)
                out["host_arrays"] = run_leg({}, args.leg_steps, host_arrays=True)
                out["host_arrays"]["arrays"] = arrays_note
                out["host_arrays"]["extra_ms_per_step"] = out["host_arrays"]["ms_per_step"] - out["ms_per_step"]
                # icicle's shape of the same call (round 6): th and rv only in every step (33.6 MB in, 33.6 MB out), the density and the
                # Courant numbers at init
                out["host_arrays_icicle"] = run_leg({}, args.leg_steps, host_arrays="thrv")
                out["host_arrays_icicle"]["arrays"] = "th, rv as host (numpy) arrays in every step: %.1f MB in, %.1f MB out; rhod and the Courant numbers at init only (kin_cloud_2d_lgrngn.hpp:242-246)" % (
                    2 * nx_tot * ny * nz * R / 1e6, 2 * nx_tot * ny * nz * R / 1e6)
                if not args.strict_fp and args.cond_solver == "lean" and not args.no_toms_leg:
                    out["api_default_host_arrays"] = run_leg({"strict_fp": False, "cond_solver": 1}, args.leg_steps, host_arrays=True)
                    out["api_default_host_arrays"]["arrays"] = arrays_note
            if not args.strict_fp and not args.no_strict_leg:
                # the opt-in parity mode (opts_init.strict_fp = 1, the API default of rounds 1-4): IEEE operation order in the condensation
                # kernel and the reference's ordered per-cell sums
                out["strict_fp"] = run_leg({"strict_fp": True}, args.strict_leg_steps)
                out["strict_fp"]["fp_mode"] = "strict IEEE order (opts_init.strict_fp = 1, opt-in)"
                out["strict_fp"]["roofline"]["kernel"] = "k_cond"
            default_box = args.sd_conc == 64 and args.workload == "stratocumulus" and args.processes == "all" and args.real == "f64"
            if default_box and not args.no_extra_legs:
                # A coalescence that COLLIDES (the stratocumulus box's candidate pairs all but never do): the Golovin test's
                # spectrum under hall_davis_no_waals, everything else as the headline -- SURVEY 8(d), C5 variant (ii)
                out["coal_stress"] = run_leg({"dry_distros": {(1e-10, 0.): lgrngn.expvolume(30.084e-6, 2 ** 23)},
                                              "kernel": lgrngn.kernel_t.hall_davis_no_waals}, args.leg_steps, collisions=True)
                out["coal_stress"]["spectrum"] = ("n(ln r) = 3 n0 (r/r0)^3 exp(-(r/r0)^3), r0 = 30.084 um, n0 = 2^23 m^-3, kappa = 1e-10 "
                                                 "(ref tests/python/physics/coalescence_golovin.py:31-44), kernel hall_davis_no_waals")
                # (round 6) a LONG window of the headline's configuration: the box long settled, 15+ storage re-orderings in it
                if args.soak_steps > 0:
                    out["soak"] = run_leg({}, args.soak_steps, listed=True)
                    out["soak"]["note"] = "the headline's options, %d steps behind 3 of warm-up on an object of its own" % args.soak_steps
                # (round 6) aerosol that KEEPS ACTIVATING: the caller swings its vapour field by +-1 % with a period of 16 steps (what an
                # updraft through cloud base does to the air that passes it; the stratocumulus box by itself settles within its first steps)
                def swing(it, f):
                    w = 2 * np.pi / 16.
                    f[1].mul_(1. + 0.01 * (np.sin(w * (it + 1)) - np.sin(w * it)))
                out["activation"] = run_leg({}, 4 * 16, forcing=swing, listed=True)
                out["activation"]["forcing"] = "rv x (1 + 0.01 sin(2 pi step / 16)) applied by the caller between steps (device arrays)"
                # BASELINE configs[1] (C2): the 2-D icicle set-up in its own arithmetic (float), th and rv as host arrays in every step
                out["c2"] = c2_leg(lgrngn, torch)
                # BASELINE configs[4] (C5): the headline spectrum x 512 per cell, 1.07e9 super-droplets on the one device (~210 GB);
                # 17 steps behind 3 of warm-up: one storage re-ordering (every 16 steps where cells are crowded) falls into them
                free_b, _tot_b = torch.cuda.mem_get_info()
                if free_b > 230e9 * (nx_tot * ny * nz) / 128. ** 3:
                    out["c5"] = run_leg({"sd_conc": 512, "n_sd_max": int(nx_tot * ny * nz * 512 * 1.15) + 1024}, 17)
                    out["c5"]["workload"] = "3-D box %dx%dx%d cells x 512 SD/cell (BASELINE configs[4]), headline options" % (nx_tot, ny, nz)
                else:
                    out["c5"] = {"skipped": "%.0f GB of device memory free, the configuration needs ~210" % (free_b / 1e9)}
        if args.full and world_out == 1 and not args.no_cpu_baseline and not args.self_ring:
            out["cpu_baseline"] = cpu_baseline(args)
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if world > 1:
        dist.all_reduce(torch.zeros(1))
        if probe_state["hung"]:                              # (an abandoned RCCL operation: do not wait for its communicator)
            # the line above is a measurement over the HOST transport of a node whose RCCL ring hung: it is printed, and the process says
            # that something was wrong (ADVICE r03 / VERDICT r04: not exit code 0)
            print("bench.py rank %d: exiting with code 4 -- the RCCL ring probe hung, the result line is the host-staged transport's" % rank,
                  file=sys.stderr, flush=True)
            sys.stdout.flush(); sys.stderr.flush()
            os._exit(4)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
