"""Comparison of windows on the device against every matrix through the host: one JSON line per shape.

On synthetic resident data (1000 individuals x 1e5 sites, --indep_geno, the MFMA kernel) two scans go through
  cmp_dist   ngd_run_windows_cmp with dist: the windows' matrices compared on the device, W (W + 2) numbers and the finished
             distances leave it
  cmp        the same without dist: W (W + 2) numbers alone
  dist       ngd_run_windows_dist alone: every matrix to the host, ngd_finish there
  host       that call followed by ngd_win_cmp_host on the host's 16 threads: the route the device tail replaces
on ONE engine, with the same arguments, in ONE process:
  plain      397 windows of 1 000 sites every 250
  wide       37 windows of 10 000 sites every 2 500
All calls return after a device synchronise, so the host clock around a call is the call.  The device forms get --warmup
calls and --reps timed ones (median reported, every run beside it); the host twin is timed --host_reps times.  The four
kernels' own device time is ngd_last_win_cmp_ms (HIP events around their launches), and the Gram kernel's share of the FP64
matrix peak and of HBM bandwidth follows from its algorithmic work: 2 W^2 P flop (half of them below the diagonal, not
computed: W (W + 1) P) and one read of the operand per tile-block row.  The two forms' Gram matrices are compared relative to
sqrt(g_aa g_bb).  A line is appended to --out as soon as its shape is done; the file is never truncated.  Not bench.py: that
one measures the flagship workload and stays as it is.

    python tools/bench_win_cmp.py [--n_ind 1000] [--n_sites 100000] [--reps 3] [--warmup 1] [--shapes plain,wide] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_MATRIX = 78.6e12  # flop/s, MI355X data sheet
PEAK_HBM = 8.0e12           # bytes/s, the same


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    runs, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        runs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(runs), runs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=100000)
    ap.add_argument("--plain_size", type=int, default=1000)
    ap.add_argument("--plain_step", type=int, default=250)
    ap.add_argument("--wide_size", type=int, default=10000)
    ap.add_argument("--wide_step", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--evol_model", type=int, default=1)
    ap.add_argument("--shapes", default="plain,wide")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "win_cmp", "bench_win_cmp.jsonl"))
    a = ap.parse_args()
    import ngsdist_amd as N

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    n, P = a.n_ind, N.n_pairs(a.n_ind)
    with N.Engine(n, a.n_sites, kernel="mfma", indep_geno=True) as e:
        e.synth_fill(1).commit()
        for shape in a.shapes.split(","):
            size, step = (a.plain_size, a.plain_step) if shape == "plain" else (a.wide_size, a.wide_step)
            lo, hi = N.window_ranges(a.n_sites, size, step)
            W = len(lo)
            ms_cd, runs_cd, got = timed(lambda: e.run_windows_cmp(lo, hi, a.evol_model), a.warmup, a.reps)
            kernels = e.last_win_cmp_ms()
            ms_c, runs_c, got_c = timed(lambda: e.run_windows_cmp(lo, hi, a.evol_model, dist=False), a.warmup, a.reps)
            ms_d, runs_d, dist = timed(lambda: e.run_windows_dist(lo, hi, a.evol_model), a.warmup, a.reps)
            assert np.array_equal(got[3].view(np.uint64), dist.view(np.uint64)) and np.array_equal(got[1].view(np.uint64), got_c[1].view(np.uint64))
            host_runs, twin_runs = [], []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                d = e.run_windows_dist(lo, hi, a.evol_model)
                t1 = time.perf_counter()
                hm, hg, hs = N.win_cmp_host(d)
                t2 = time.perf_counter()
                host_runs.append((t2 - t0) * 1e3)
                twin_runs.append((t2 - t1) * 1e3)
            ok = got[2] == 1
            scale = np.sqrt(np.outer(np.diag(hg), np.diag(hg)))[np.ix_(ok, ok)]
            diff = float((np.abs(got[1] - hg)[np.ix_(ok, ok)] / scale).max())
            s = N.win_cmp_slice(W, P)
            n_g = (W + 15) // 16
            T = min(4, n_g)
            n_br = (n_g + T - 1) // T
            flop = W * (W + 1) * P  # the triangle with its diagonal, a multiply and an add per cell
            read = n_br * (n_br + 1) // 2 * 2 * T * 16 * P * 8  # every tile block reads its T row and T column groups once
            gram_s = kernels["gram"] * 1e-3
            line = {
                "shape": shape, "n_ind": n, "n_sites": a.n_sites, "win_size": size, "win_step": step, "windows": W, "cells": P,
                "slice_cells": s, "slices": (P + s - 1) // s, "status_1": int(ok.sum()),
                "cmp_dist_ms": ms_cd, "cmp_dist_ms_runs": runs_cd, "cmp_ms": ms_c, "cmp_ms_runs": runs_c,
                "dist_ms": ms_d, "dist_ms_runs": runs_d, "host_route_ms": statistics.median(host_runs), "host_route_ms_runs": host_runs,
                "host_twin_part_ms_runs": twin_runs, "kernel_ms": kernels,
                "gram_flop": flop, "gram_tflops": flop / gram_s / 1e12, "gram_share_of_fp64_matrix_peak": flop / gram_s / PEAK_FP64_MATRIX,
                "gram_operand_bytes_by_tile_blocks": read, "gram_operand_bytes_once": W * P * 8,
                "gram_share_of_hbm_peak_by_tile_blocks": read / gram_s / PEAK_HBM, "gram_share_of_hbm_peak_once": W * P * 8 / gram_s / PEAK_HBM,
                "bytes_to_host_cmp": W * (W + 1) * 8 + W * 4, "bytes_to_host_cmp_dist": W * (W + 1) * 8 + W * 4 + W * P * 16,
                "bytes_to_host_host_route": W * P * 16, "gram_device_vs_host_twin": diff,
            }
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
