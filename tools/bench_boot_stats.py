"""Bootstrap summaries on the device against every replicate on the host: one JSON line per shape.

On synthetic resident data (1000 individuals x 1e5 sites, --indep_geno, the MFMA kernel) two jobs go through their *_dist
form -- all R + 1 matrices of every set to the host, ngd_finish on its threads, the statistics still the caller's to
compute -- and through their *_stats form -- five doubles and a count per cell leave the device -- on ONE engine, with the
same arguments, in ONE process, into buffers made and touched beforehand:
  windows   37 windows of 10 000 sites every 2 500, R = 100 replicates inside each, blocks of 100 sites
            (ngd_run_windows_job_var_dist / ngd_run_windows_job_var_stats)
  job       the whole data set and 100 replicates, blocks of 100 sites (ngd_run_job_dist / ngd_run_job_stats)
Both calls return after a device synchronise, so the host clock around a call is the call.  Each form gets --warmup calls,
then the two alternate --reps times; the median of each is reported with every run beside it.  The summary kernel's own
device time (ngd_last_boot_stats_ms: HIP events around its launches) gives its bytes/s at 16 bytes read per (cell, matrix)
and 48 written per cell, and its share of the 6.29 TB/s a copy kernel reaches on an MI355X (8.0 TB/s by specification).
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/bench_boot_stats.py [--n_ind 1000] [--n_sites 100000] [--n_rep 100] [--reps 5] [--warmup 1] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12  # bytes/s: a float4 copy kernel on an MI355X; the specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=100000)
    ap.add_argument("--n_rep", type=int, default=100)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--win_size", type=int, default=10000)
    ap.add_argument("--win_step", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of each form (the median is reported)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--evol_model", type=int, default=1)
    ap.add_argument("--ci", type=float, default=0.95)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boot_stats", "bench_boot_stats.jsonl"))
    args = ap.parse_args()
    import ngsdist_amd as N

    if N.device_count() < 1:
        sys.exit("bench_boot_stats: no HIP device (nothing is measured without one)")
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    R, q, n_mat = args.n_rep, args.block, args.n_rep + 1
    lines = []
    with N.Engine(args.n_ind, args.n_sites, indep_geno=True, kernel="mfma") as e:
        e.synth_fill(3, 0.0)
        L, h, n_pairs = e._L, e._h, e.n_pairs
        lo, hi = N.window_ranges(e.n_sites, args.win_size, args.win_step)
        n_win = int(len(lo))
        wmaps, woff = N.window_boot_maps(5, lo, hi, R, q)
        t = N.Taus(5)
        jmaps = np.ascontiguousarray(np.stack([t.block_map(e.n_sites // q) for _ in range(R)]), dtype=np.uint64)
        lp, hp, mp, op = (a.ctypes.data_as(up) for a in (lo, hi, wmaps, woff))
        shapes = {
            "windows": (n_win,
                        lambda d: L.ngd_run_windows_job_var_dist(h, lp, hp, n_win, mp, wmaps.size, op, R, q, 0, args.evol_model, d),
                        lambda s, u: L.ngd_run_windows_job_var_stats(h, lp, hp, n_win, mp, wmaps.size, op, R, q, 0, args.evol_model,
                                                                     args.ci, s, u)),
            "job": (1,
                    lambda d: L.ngd_run_job_dist(h, jmaps.ctypes.data_as(up), R, jmaps.shape[1], q, 0, args.evol_model, d),
                    lambda s, u: L.ngd_run_job_stats(h, jmaps.ctypes.data_as(up), R, jmaps.shape[1], q, 0, args.evol_model, args.ci, s, u)),
        }
        for name, (n_set, f_dist, f_stats) in shapes.items():
            dist = np.zeros((n_set, n_mat, n_pairs))  # (touched: no page faults inside the timed calls)
            stats = np.zeros((n_set, 5, n_pairs))
            used = np.zeros((n_set, n_pairs), dtype=np.uint64)

            def call_dist():
                t0 = time.perf_counter()
                rc = f_dist(dist.ctypes.data_as(dp))
                assert rc == 0, L.ngd_last_error()
                return (time.perf_counter() - t0) * 1e3

            def call_stats():
                t0 = time.perf_counter()
                rc = f_stats(stats.ctypes.data_as(dp), used.ctypes.data_as(up))
                assert rc == 0, L.ngd_last_error()
                return (time.perf_counter() - t0) * 1e3, e.last_boot_stats_ms()

            for _ in range(args.warmup):
                call_dist()
                call_stats()
            t_dist, t_stats, t_kern = [], [], []
            for _ in range(args.reps):  # alternating: both forms see the same machine
                t_dist.append(call_dist())
                w, k = call_stats()
                t_stats.append(w)
                t_kern.append(k)
            kern = statistics.median(t_kern)
            cells = n_set * n_pairs
            moved = cells * (n_mat * 16 + 48)
            rate = moved / (kern * 1e-3) if kern else None
            # the statistics of one cell the host's way from the _dist call's matrices (a sanity check, not the test)
            col = dist[0, 1:, 7]
            col = col[np.isfinite(col)]
            out = {"shape": name, "n_ind": args.n_ind, "n_sites": int(e.n_sites), "n_set": n_set, "n_rep": R, "block_size": q,
                   "win_size": args.win_size if name == "windows" else None, "win_step": args.win_step if name == "windows" else None,
                   "evol_model": args.evol_model, "ci": args.ci, "warmup": args.warmup, "reps": args.reps,
                   "dist_ms_median": round(statistics.median(t_dist), 3), "stats_ms_median": round(statistics.median(t_stats), 3),
                   "stats_over_dist": round(statistics.median(t_stats) / statistics.median(t_dist), 4),
                   "dist_ms_runs": [round(x, 3) for x in t_dist], "stats_ms_runs": [round(x, 3) for x in t_stats],
                   "kernel_device_ms_median": round(kern, 4), "kernel_device_ms_runs": [round(x, 4) for x in t_kern],
                   "cells": cells, "kernel_bytes": moved, "kernel_bytes_per_s": round(rate, 1) if rate else None,
                   "share_of_hbm_measured_6.29e12": round(rate / HBM_MEASURED, 4) if rate else None,
                   "share_of_hbm_spec_8e12": round(rate / HBM_SPEC, 4) if rate else None,
                   "dist_bytes_to_host": cells * n_mat * 16, "stats_bytes_to_host": int(stats.nbytes + used.nbytes),
                   "mean_cell_7": float(stats[0, 1, 7]), "mean_cell_7_from_dist": float(np.mean(col)) if col.size else None}
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            del dist, stats, used
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
