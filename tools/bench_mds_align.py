"""Aligned MDS replicates on the device against the same work through the host: one JSON line.

On synthetic resident data (1000 individuals x 1e5 sites, --indep_geno, the MFMA kernel), 37 windows of 10 000 sites every
2 500 with R = 100 replicates inside each, blocks of 100 sites, K = 4 -- 3 737 matrices -- go
  aligned   through ngd_run_windows_job_var_mds_align: MDS, alignment and summaries on the device; matrix 0 of every set,
            5 K (n + 1) statistics and R + 1 fits per set leave it (aligned = NULL)
  host      through ngd_run_windows_job_var_mds -- K (n + 1) + 2 numbers of EVERY matrix leave the device --, then
            ngd_mds_align_host and ngd_boot_stats_host on the host's threads (the cells put together by numpy in between:
            timed apart, host_gather_ms)
on ONE engine, with the same arguments, in ONE process, into buffers made and touched beforehand, the two forms taking turns:
--warmup rounds, then --reps timed ones (medians reported, every run beside them).  All calls return after a device
synchronise, so the host clock around a call is the call.  The kernels' own device time is HIP events around their
launches: ngd_last_mds_ms, ngd_last_mds_align_ms (k_mds_coords + k_mds_align), ngd_last_boot_stats_ms.  The two forms'
statistics are compared relative to the largest |coordinate| of matrix 0.  With --plain_only the script times
ngd_run_windows_job_var_mds alone, through the package of --root: another build of the library (the parent commit's, for
the same-session figure the aligned call is held against).  A line is appended to --out; the file is never truncated.  Not
bench.py: that one measures the flagship workload and stays as it is.

    python tools/bench_mds_align.py [--n_ind 1000] [--n_sites 100000] [--n_rep 100] [--dim 4] [--reps 3] [--warmup 1]
                                    [--plain_only] [--root DIR] [--label TEXT] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=100000)
    ap.add_argument("--n_rep", type=int, default=100)
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--win_size", type=int, default=10000)
    ap.add_argument("--win_step", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--evol_model", type=int, default=1)
    ap.add_argument("--ci", type=float, default=0.95)
    ap.add_argument("--plain_only", action="store_true", help="time ngd_run_windows_job_var_mds alone")
    ap.add_argument("--root", default=ROOT, help="the tree whose ngsdist_amd package is measured")
    ap.add_argument("--label", default="", help="a word for the line (which build)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mds", "bench_mds_align.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ngsdist_amd as N

    if N.device_count() < 1:
        sys.exit("bench_mds_align: no HIP device (nothing is measured without one)")
    dp, up, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    R, q, n, model, K, ci = args.n_rep, args.block, args.n_ind, args.evol_model, args.dim, args.ci
    n_mat, n_cells = R + 1, K * (n + 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with N.Engine(n, args.n_sites, indep_geno=True, kernel="mfma") as e:
        e.synth_fill(3, 0.0)
        L, h, n_pairs = e._L, e._h, e.n_pairs
        lo, hi = N.window_ranges(e.n_sites, args.win_size, args.win_step)
        wmaps, woff = N.window_boot_maps(5, lo, hi, R, q)
        lp, hp, mp, op = (a.ctypes.data_as(up) for a in (lo, hi, wmaps, woff))
        n_set = int(len(lo))
        tot = n_set * n_mat
        # (touched: no page faults inside the timed calls)
        eig, vec, tt, status = np.zeros((n_set, n_mat, K)), np.zeros((n_set, n_mat, K, n)), np.zeros((n_set, n_mat, 2)), np.zeros((n_set, n_mat), dtype=np.uint32)
        dist0 = np.zeros((n_set, n_pairs))

        def call_plain():
            t0 = time.perf_counter()
            rc = L.ngd_run_windows_job_var_mds(h, lp, hp, n_set, mp, wmaps.size, op, R, q, 0, model, K, eig.ctypes.data_as(dp),
                                               vec.ctypes.data_as(dp), tt.ctypes.data_as(dp), status.ctypes.data_as(u32p), dist0.ctypes.data_as(dp))
            assert rc == 0, L.ngd_last_error()
            return (time.perf_counter() - t0) * 1e3, e.last_mds_ms()

        line = {"shape": "windows", "label": args.label, "n_ind": n, "n_sites": int(e.n_sites), "n_set": n_set, "n_mat_per_set": n_mat,
                "matrices": tot, "K": K, "block_size": q, "evol_model": model, "ci": ci, "warmup": args.warmup, "reps": args.reps}
        plain_bytes = int(eig.nbytes + vec.nbytes + tt.nbytes + status.nbytes + n_set * n_pairs * 16)
        if args.plain_only:
            for _ in range(args.warmup):
                call_plain()
            runs = [call_plain() for _ in range(args.reps)]
            line.update({"mds_ms_median": round(statistics.median(r[0] for r in runs), 3), "mds_ms_runs": [round(r[0], 3) for r in runs],
                         "mds_kernel_ms_median": round(statistics.median(r[1] for r in runs), 3), "mds_bytes_to_host": plain_bytes})
        else:
            eig0, vec0, tot0 = np.zeros((n_set, K)), np.zeros((n_set, K, n)), np.zeros((n_set, 2))
            stats, used, fit = np.zeros((n_set, 5, n_cells)), np.zeros(n_set, dtype=np.uint64), np.zeros((n_set, n_mat))
            hal, hfit = np.zeros((n_set, n_mat, K, n)), np.zeros((n_set, n_mat))
            hstats, hused = np.zeros((n_set, 5, n_cells)), np.zeros((n_set, n_cells), dtype=np.uint64)
            cells = np.zeros((n_set, n_mat, n_cells))

            def call_aligned():
                t0 = time.perf_counter()
                rc = L.ngd_run_windows_job_var_mds_align(h, lp, hp, n_set, mp, wmaps.size, op, R, q, 0, model, K, ci, eig0.ctypes.data_as(dp),
                                                         vec0.ctypes.data_as(dp), tot0.ctypes.data_as(dp), status.ctypes.data_as(u32p),
                                                         stats.ctypes.data_as(dp), used.ctypes.data_as(up), fit.ctypes.data_as(dp), None,
                                                         dist0.ctypes.data_as(dp))
                assert rc == 0, L.ngd_last_error()
                return (time.perf_counter() - t0) * 1e3, e.last_mds_ms(), e.last_mds_align_ms(), e.last_boot_stats_ms()

            def call_host():
                w, k = call_plain()
                t0 = time.perf_counter()
                rc = L.ngd_mds_align_host(eig.ctypes.data_as(dp), vec.ctypes.data_as(dp), status.ctypes.data_as(u32p), n_set, n_mat, n, K,
                                          hal.ctypes.data_as(dp), hfit.ctypes.data_as(dp))
                assert rc == 0
                t1 = time.perf_counter()
                cells[:, :, :K * n] = hal.reshape(n_set, n_mat, K * n)
                cells[:, :, K * n:] = np.where(np.isnan(hfit)[..., None], np.nan, eig)
                t2 = time.perf_counter()
                rc = L.ngd_boot_stats_host(cells.ctypes.data_as(dp), n_set, n_mat, n_cells, ci, hstats.ctypes.data_as(dp), hused.ctypes.data_as(up))
                assert rc == 0
                t3 = time.perf_counter()
                return w + (t3 - t0) * 1e3, w, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3

            for _ in range(args.warmup):
                call_aligned()
                call_host()
            a_runs, h_runs = [], []
            for _ in range(args.reps):
                a_runs.append(call_aligned())
                h_runs.append(call_host())
            scale = np.abs(vec0 * np.sqrt(np.maximum(eig0, 0))[..., None]).max()
            both = np.isfinite(stats) & np.isfinite(hstats)
            med = lambda runs, k: round(statistics.median(r[k] for r in runs), 3)
            line.update({
                "host_threads": min(16, os.cpu_count() or 1),
                "aligned_ms_median": med(a_runs, 0), "aligned_ms_runs": [round(r[0], 3) for r in a_runs],
                "aligned_mds_kernel_ms_median": med(a_runs, 1), "align_kernels_ms_median": med(a_runs, 2),
                "align_kernels_ms_runs": [round(r[2], 3) for r in a_runs], "boot_stats_kernel_ms_median": med(a_runs, 3),
                "host_route_ms_median": med(h_runs, 0), "host_route_ms_runs": [round(r[0], 3) for r in h_runs],
                "mds_ms_median": med(h_runs, 1), "mds_ms_runs": [round(r[1], 3) for r in h_runs],
                "host_align_ms_median": med(h_runs, 2), "host_gather_ms_median": med(h_runs, 3), "host_boot_stats_ms_median": med(h_runs, 4),
                "aligned_over_mds": round(med(a_runs, 0) / med(h_runs, 1), 4), "aligned_over_host_route": round(med(a_runs, 0) / med(h_runs, 0), 4),
                "aligned_bytes_to_host": int(eig0.nbytes + vec0.nbytes + tot0.nbytes + status.nbytes + stats.nbytes + n_set * n_cells * 8 +
                                             fit.nbytes + n_set * n_pairs * 16),
                "mds_bytes_to_host": plain_bytes,
                "sets_used": [int(used.min()), int(used.max())],
                "same_nan_pattern": bool(np.array_equal(np.isnan(stats), np.isnan(hstats))),
                "max_stat_diff_over_largest_coordinate": float(np.abs(stats[both] - hstats[both]).max() / scale),
                "max_fit_diff_relative": float(np.nanmax(np.abs(fit - hfit) / np.maximum(np.abs(hfit), 1e-300)))})
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
