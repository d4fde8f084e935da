"""Group means on the device against the n x n tail on the host: one JSON line per (window shape, grouping).

On synthetic resident data (1000 individuals x 1e5 sites, --indep_geno, the MFMA kernel) the same windows go through
ngd_run_windows_dist -- every matrix to the host, ngd_finish on its threads -- and through ngd_run_windows_groups -- the
G x G means reduced on the device -- in ONE process, into buffers made and touched beforehand.  Both calls return after a
device synchronise, so the host clock around a call is the call.  Each gets --warmup calls, then the two alternate --reps
times and the median of each is reported with every run beside it.  Shapes: windows of 10 000 sites every 2 500 (37) and of
1 000 every 250 (397); 4 contiguous groups and 4 interleaved ones (i % 4).  The reduction's own device time
(ngd_last_groups_ms: HIP events around its kernels) gives its achieved bytes/s at 16 bytes per cell (sum and count), 8 with
--tot_sites.  Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/bench_groups.py [--n_ind 1000] [--n_sites 100000] [--reps 10] [--warmup 3] [--tot_sites 0]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10, help="timed calls of each form (at least 10; the median is reported)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tot_sites", type=int, default=0)
    ap.add_argument("--evol_model", type=int, default=1)
    args = ap.parse_args()
    import ngsdist_amd as N

    if N.device_count() < 1:
        sys.exit("bench_groups: no HIP device (nothing is measured without one)")
    reps = max(10, args.reps)
    n, G = args.n_ind, 4
    groupings = {"contiguous": np.arange(n) * G // n, "interleaved": np.arange(n) % G}
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    with N.Engine(n, args.n_sites, indep_geno=True, kernel="mfma") as e:
        e.synth_fill(3, 0.0)
        L, h = e._L, e._h
        for size, step in ((10000, 2500), (1000, 250)):
            lo, hi = N.window_ranges(e.n_sites, size, step)
            n_win = int(len(lo))
            lp, hp = lo.ctypes.data_as(up), hi.ctypes.data_as(up)
            dist = np.zeros((n_win, e.n_pairs))  # (touched: no page faults inside the timed calls)
            mean = np.zeros((n_win, N.n_group_pairs(G)))
            used = np.zeros(mean.shape, dtype=np.uint64)

            def call_dist():
                t0 = time.perf_counter()
                rc = L.ngd_run_windows_dist(h, lp, hp, n_win, args.tot_sites, args.evol_model, dist.ctypes.data_as(dp))
                assert rc == 0, L.ngd_last_error()
                return (time.perf_counter() - t0) * 1e3

            def call_groups():
                t0 = time.perf_counter()
                rc = L.ngd_run_windows_groups(h, lp, hp, n_win, args.tot_sites, args.evol_model, mean.ctypes.data_as(dp),
                                              used.ctypes.data_as(up))
                assert rc == 0, L.ngd_last_error()
                return (time.perf_counter() - t0) * 1e3, e.groups_ms(), e.windows_info()["ms"]

            for name, g in groupings.items():
                e.set_groups(g, G)
                for _ in range(args.warmup):
                    call_dist()
                    call_groups()
                t_dist, t_grp, t_kern, t_pass = [], [], [], []
                for _ in range(reps):  # alternating: both forms see the same machine
                    t_dist.append(call_dist())
                    w, k, p = call_groups()
                    t_grp.append(w)
                    t_kern.append(k)
                    t_pass.append(p)
                cells = int(N.group_cells(g, G).sum()) * n_win
                per_cell = 8 if args.tot_sites else 16
                kern = statistics.median(t_kern)
                # the groups' means against the n x n matrices of the _dist call, the host's way (a sanity check, not the test)
                a, b = np.triu_indices(n, 1)
                gp0 = np.flatnonzero((g[a] == 0) & (g[b] == 0))
                ref = float(np.mean(dist[0, gp0][np.isfinite(dist[0, gp0])]))
                out = {"n_ind": n, "n_sites": e.n_sites, "win_size": size, "win_step": step, "n_win": n_win, "groups": G,
                       "grouping": name, "evol_model": args.evol_model, "tot_sites": args.tot_sites, "warmup": args.warmup, "reps": reps,
                       "dist_ms_median": round(statistics.median(t_dist), 3), "groups_ms_median": round(statistics.median(t_grp), 3),
                       "groups_over_dist": round(statistics.median(t_grp) / statistics.median(t_dist), 4),
                       "dist_ms_runs": [round(x, 3) for x in t_dist], "groups_ms_runs": [round(x, 3) for x in t_grp],
                       "accumulation_device_ms_median": round(statistics.median(t_pass), 3),
                       "reduce_kernels_device_ms_median": round(kern, 4), "reduce_kernels_device_ms_runs": [round(x, 4) for x in t_kern],
                       "cells": cells, "bytes_per_cell": per_cell,
                       "reduce_bytes_per_s": round(cells * per_cell / (kern * 1e-3), 1) if kern else None,
                       "dist_bytes_to_host": n_win * e.n_pairs * 16,
                       "groups_bytes_to_host": int(mean.nbytes + used.nbytes),
                       "mean_0_0_window_0": float(mean[0, 0]), "mean_0_0_window_0_from_dist": ref}
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
