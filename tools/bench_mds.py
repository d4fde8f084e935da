"""Classical MDS on the device against every matrix through the host: one JSON line per shape.

On synthetic resident data (1000 individuals x 1e5 sites, --indep_geno, the MFMA kernel) three jobs go through their *_dist
form followed by ngd_mds_host on the host's threads -- every matrix to the host, ngd_finish, then the O(n^3)
tridiagonalisation there: the route the device tail replaces -- and through their *_mds form -- K (n + 1) + 2 numbers per
matrix and matrix 0 of every set leave the device -- on ONE engine, with the same arguments, in ONE process, into buffers
made and touched beforehand, all at K = 4; a fourth is the least a call can hold:
  job       the whole data set and 100 replicates, blocks of 100 sites (ngd_run_job_dist / ngd_run_job_mds): 101 matrices
  plain     397 windows of 1 000 sites every 250, no replicates (ngd_run_windows_dist / ngd_run_windows_mds)
  windows   37 windows of 10 000 sites every 2 500, R = 100 replicates inside each, blocks of 100 sites
            (ngd_run_windows_job_var_dist / ngd_run_windows_job_var_mds): 3 737 matrices
  single    the whole data set alone, no replicates (ngd_run_job_dist / ngd_run_job_mds with n_rep 0): ONE matrix, where
            ngd_mds_host has one thread's work and the device one workgroup's; both forms timed --reps times
All calls return after a device synchronise, so the host clock around a call is the call.  The device form gets --warmup
calls and --reps timed ones (median reported, every run beside it).  Of the host form the _dist part is warmed up alike and
ngd_mds_host once on up to 16 of the shape's matrices (the pool's threads started, its code paged in); the whole form is then
timed --host_reps times (the line carries every run and the twin's part of each: host_mds_part_ms_runs).  With
--host_max_mat M the host twin of a shape with more matrices runs on the first M of them only and the line says so
(host_mds_matrices, host_route_ms_scaled: the _dist part as measured plus the twin's time scaled by matrices / M -- an
estimate, marked as one).  The MDS kernel's own device time is ngd_last_mds_ms (HIP events around its launches).  The two
forms' eigenvalues are compared relative to the largest of each matrix.  --wg_sweep times the kernel of the first shape at
workgroups of 256, 512 and 1024 threads (NGD_MDS_WG), in alternating rounds.  A line is appended to --out as soon as its
shape is done; the file is never truncated (runs of single shapes add up; start from no file for a fresh record).  Not
bench.py: that one measures the flagship workload and stays as it is.

    python tools/bench_mds.py [--n_ind 1000] [--n_sites 100000] [--n_rep 100] [--dim 4] [--reps 3] [--warmup 1]
                              [--shapes job,plain,windows,single] [--host_max_mat 0] [--wg_sweep] [--out FILE]
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
    ap.add_argument("--n_rep", type=int, default=100)
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--win_size", type=int, default=10000)
    ap.add_argument("--win_step", type=int, default=2500)
    ap.add_argument("--plain_size", type=int, default=1000)
    ap.add_argument("--plain_step", type=int, default=250)
    ap.add_argument("--reps", type=int, default=3, help="timed calls of the device form (the median is reported)")
    ap.add_argument("--host_reps", type=int, default=1, help="timed calls of the host form")
    ap.add_argument("--host_max_mat", type=int, default=0, help="the host twin runs on at most this many matrices (0: all)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--evol_model", type=int, default=1)
    ap.add_argument("--shapes", default="job,plain,windows,single")
    ap.add_argument("--wg_sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mds", "bench_mds.jsonl"))
    args = ap.parse_args()
    import ngsdist_amd as N

    if N.device_count() < 1:
        sys.exit("bench_mds: no HIP device (nothing is measured without one)")
    dp, up, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    R, q, n, model, K = args.n_rep, args.block, args.n_ind, args.evol_model, args.dim
    threads = min(16, os.cpu_count() or 1)  # ngd_mds_host's pool: the caller and up to 15 workers
    wg_default = int(os.environ.get("NGD_MDS_WG", "1024"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with N.Engine(n, args.n_sites, indep_geno=True, kernel="mfma") as e:
        e.synth_fill(3, 0.0)
        L, h, n_pairs = e._L, e._h, e.n_pairs
        lo, hi = N.window_ranges(e.n_sites, args.win_size, args.win_step)
        plo, phi = N.window_ranges(e.n_sites, args.plain_size, args.plain_step)
        wmaps, woff = N.window_boot_maps(5, lo, hi, R, q)
        t = N.Taus(5)
        jmaps = np.ascontiguousarray(np.stack([t.block_map(e.n_sites // q) for _ in range(R)]), dtype=np.uint64)
        lp, hp, mp, op, plp, php = (a.ctypes.data_as(up) for a in (lo, hi, wmaps, woff, plo, phi))
        jp = jmaps.ctypes.data_as(up)
        shapes = {
            "job": (1, R + 1,
                    lambda d: L.ngd_run_job_dist(h, jp, R, jmaps.shape[1], q, 0, model, d),
                    lambda *o: L.ngd_run_job_mds(h, jp, R, jmaps.shape[1], q, 0, model, K, *o)),
            "windows": (int(len(lo)), R + 1,
                        lambda d: L.ngd_run_windows_job_var_dist(h, lp, hp, len(lo), mp, wmaps.size, op, R, q, 0, model, d),
                        lambda *o: L.ngd_run_windows_job_var_mds(h, lp, hp, len(lo), mp, wmaps.size, op, R, q, 0, model, K, *o)),
            "single": (1, 1,
                       lambda d: L.ngd_run_job_dist(h, None, 0, 0, q, 0, model, d),
                       lambda *o: L.ngd_run_job_mds(h, None, 0, 0, q, 0, model, K, *o)),
            "plain": (int(len(plo)), 1,
                      lambda d: L.ngd_run_windows_dist(h, plp, php, len(plo), 0, model, d),
                      lambda *o: L.ngd_run_windows_mds(h, plp, php, len(plo), 0, model, K, *o)),
        }
        for name in [s for s in args.shapes.split(",") if s]:
            n_set, n_mat, f_dist, f_mds = shapes[name]
            tot = n_set * n_mat
            n_host = min(tot, args.host_max_mat) if args.host_max_mat else tot
            dist = np.zeros((tot, n_pairs))  # (touched: no page faults inside the timed calls)
            eig, vec, tt, status = np.zeros((tot, K)), np.zeros((tot, K, n)), np.zeros((tot, 2)), np.zeros(tot, dtype=np.uint32)
            heig, hvec, htt, hstatus = np.zeros((n_host, K)), np.zeros((n_host, K, n)), np.zeros((n_host, 2)), np.zeros(n_host, dtype=np.uint32)
            dist0 = np.zeros((n_set, n_pairs))

            def call_host():
                t0 = time.perf_counter()
                rc = f_dist(dist.ctypes.data_as(dp))
                assert rc == 0, L.ngd_last_error()
                t1 = time.perf_counter()
                rc = L.ngd_mds_host(dist.ctypes.data_as(dp), n_host, n, K, heig.ctypes.data_as(dp), hvec.ctypes.data_as(dp),
                                    htt.ctypes.data_as(dp), hstatus.ctypes.data_as(u32p))
                assert rc == 0
                return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3

            def warm_host():  # (after a _dist call: the twin on a few of the matrices, so that no timed call starts the pool)
                k = min(n_host, 16)
                rc = L.ngd_mds_host(dist.ctypes.data_as(dp), k, n, K, heig.ctypes.data_as(dp), hvec.ctypes.data_as(dp),
                                    htt.ctypes.data_as(dp), hstatus.ctypes.data_as(u32p))
                assert rc == 0

            def call_mds():
                t0 = time.perf_counter()
                rc = f_mds(eig.ctypes.data_as(dp), vec.ctypes.data_as(dp), tt.ctypes.data_as(dp), status.ctypes.data_as(u32p),
                           dist0.ctypes.data_as(dp))
                assert rc == 0, L.ngd_last_error()
                return (time.perf_counter() - t0) * 1e3, e.last_mds_ms()

            for _ in range(args.warmup):
                call_mds()
                assert f_dist(dist.ctypes.data_as(dp)) == 0, L.ngd_last_error()  # (the host form's device part, warmed up alike)
                warm_host()
            t_mds, t_kern = [], []
            for _ in range(args.reps):
                w, k = call_mds()
                t_mds.append(w)
                t_kern.append(k)
            t_host, t_dist = [], []
            for _ in range(max(args.host_reps, args.reps) if tot == 1 else args.host_reps):
                w, d = call_host()
                t_host.append(w)
                t_dist.append(d)
            ok = (status[:n_host] == 1) & (hstatus == 1)
            scale = np.abs(heig[ok]).max(axis=1, keepdims=True)
            eig_diff = float((np.abs(eig[:n_host][ok] - heig[ok]) / scale).max()) if ok.any() else None
            dots = float(np.abs((vec[:n_host][ok] * hvec[ok]).sum(axis=2)).min()) if ok.any() else None
            sweep = None
            if args.wg_sweep and name == args.shapes.split(",")[0]:
                sweep = {256: [], 512: [], 1024: []}
                for _ in range(args.reps):
                    for wg in sweep:
                        os.environ["NGD_MDS_WG"] = str(wg)
                        sweep[wg].append(round(call_mds()[1], 3))
                os.environ["NGD_MDS_WG"] = str(wg_default)
                sweep = {str(k): {"kernel_ms_median": statistics.median(v), "kernel_ms_runs": v} for k, v in sweep.items()}
            # what the method needs of the kernel: per Householder step the trailing block read for p = S v, read and written for
            # the rank-2 update -- 3 * 8 bytes per cell of the block, summed over the steps
            cells = sum(m * m for m in range(2, n))
            kern_s = statistics.median(t_kern) * 1e-3
            host_ms, dist_ms = statistics.median(t_host), statistics.median(t_dist)
            scaled = dist_ms + (host_ms - dist_ms) * tot / n_host
            out = {"shape": name, "n_ind": n, "n_sites": int(e.n_sites), "n_set": n_set, "n_mat_per_set": n_mat, "matrices": tot, "K": K,
                   "block_size": q if n_mat > 1 else None, "evol_model": model, "warmup": args.warmup, "reps": args.reps,
                   "host_reps": len(t_host), "host_threads": threads, "workgroup": wg_default,
                   "mds_ms_median": round(statistics.median(t_mds), 3), "mds_ms_runs": [round(x, 3) for x in t_mds],
                   "host_mds_matrices": n_host,
                   "dist_then_host_mds_ms_median": round(host_ms, 3), "dist_then_host_mds_ms_runs": [round(x, 3) for x in t_host],
                   "dist_part_ms_runs": [round(x, 3) for x in t_dist],
                   "host_mds_part_ms_runs": [round(a - b, 3) for a, b in zip(t_host, t_dist)],
                   "host_route_ms_scaled": round(scaled, 3), "host_route_is_estimate": n_host != tot,
                   "mds_over_host": round(statistics.median(t_mds) / scaled, 4),
                   "kernel_device_ms_median": round(statistics.median(t_kern), 3), "kernel_device_ms_runs": [round(x, 3) for x in t_kern],
                   "kernel_ms_per_matrix": round(statistics.median(t_kern) / tot, 4),
                   "host_bytes_to_host": tot * n_pairs * 16,
                   "mds_bytes_to_host": int(eig.nbytes + vec.nbytes + tt.nbytes + status.nbytes + n_set * n_pairs * 16),
                   "matrices_with_status_1": int(status.sum()),
                   "kernel_scratch_bytes_needed": 24 * cells * int(status.sum()),
                   "kernel_scratch_bytes_per_s": round(24 * cells * int(status.sum()) / kern_s, 1) if kern_s else None,
                   "max_eig_diff_over_largest_vs_host": eig_diff, "min_abs_dot_with_host_vectors": dots, "wg_sweep": sweep}
            with open(args.out, "a") as f:
                f.write(json.dumps(out) + "\n")
            print(json.dumps(out), flush=True)
            del dist, eig, vec, tt, status, heig, hvec, htt, hstatus, dist0


if __name__ == "__main__":
    main()
