"""Neighbour-joining trees on the device against every matrix through the host: one JSON line per shape.

On synthetic resident data (1000 individuals x 1e5 sites, --indep_geno, the MFMA kernel) three jobs go through their *_dist
form followed by ngd_nj_host on the host's threads -- every matrix to the host, ngd_finish, then the O(n^3) joins there --
and through their *_nj form -- 2 n - 3 branches per matrix and matrix 0 of every set leave the device -- on ONE engine, with
the same arguments, in ONE process, into buffers made and touched beforehand:
  job       the whole data set and 100 replicates, blocks of 100 sites (ngd_run_job_dist / ngd_run_job_nj): 101 matrices
  windows   37 windows of 10 000 sites every 2 500, R = 100 replicates inside each, blocks of 100 sites
            (ngd_run_windows_job_var_dist / ngd_run_windows_job_var_nj): 3 737 matrices
  plain     397 windows of 1 000 sites every 250, no replicates (ngd_run_windows_dist / ngd_run_windows_nj)
All calls return after a device synchronise, so the host clock around a call is the call.  The device form gets --warmup
calls and --reps timed ones (median reported, every run beside it); the host form, minutes long at the second shape, is
timed --host_reps times.  The tree kernel's own device time is ngd_last_nj_ms (HIP events around its launches).  The two
forms' records are compared: model 0 would be bit for bit, under models 1 and 2 the device's log may pick the other record
at an m = 4 tie, so the line carries the number of matrices whose records are equal and whose bipartitions are.
--wg_sweep times the kernel of the first shape at workgroups of 256, 512 and 1024 threads (NGD_NJ_WG), in alternating rounds.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/bench_nj.py [--n_ind 1000] [--n_sites 100000] [--n_rep 100] [--reps 3] [--warmup 1] [--shapes job,windows,plain]
                             [--wg_sweep] [--out FILE]
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


def splits(child, n):
    """the bipartitions of a record's joins: leaf sets as bit masks, on the side without leaf 0"""
    under = [1 << k for k in range(n)]
    full = (1 << n) - 1
    for t in range(n - 3):
        under.append(under[int(child[2 * t])] | under[int(child[2 * t + 1])])
    return {m ^ full if m & 1 else m for m in under[n:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=100000)
    ap.add_argument("--n_rep", type=int, default=100)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--win_size", type=int, default=10000)
    ap.add_argument("--win_step", type=int, default=2500)
    ap.add_argument("--plain_size", type=int, default=1000)
    ap.add_argument("--plain_step", type=int, default=250)
    ap.add_argument("--reps", type=int, default=3, help="timed calls of the device form (the median is reported)")
    ap.add_argument("--host_reps", type=int, default=1, help="timed calls of the host form")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--evol_model", type=int, default=1)
    ap.add_argument("--shapes", default="job,windows,plain")
    ap.add_argument("--wg_sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nj", "bench_nj.jsonl"))
    args = ap.parse_args()
    import ngsdist_amd as N

    if N.device_count() < 1:
        sys.exit("bench_nj: no HIP device (nothing is measured without one)")
    dp, up, ip, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    R, q, n, model = args.n_rep, args.block, args.n_ind, args.evol_model
    nb = 2 * n - 3
    threads = min(16, os.cpu_count() or 1)  # ngd_nj_host's pool: the caller and up to 15 workers
    wg_default = int(os.environ.get("NGD_NJ_WG", "1024"))
    lines = []
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
                    lambda c, l, s, d0: L.ngd_run_job_nj(h, jp, R, jmaps.shape[1], q, 0, model, c, l, s, d0)),
            "windows": (int(len(lo)), R + 1,
                        lambda d: L.ngd_run_windows_job_var_dist(h, lp, hp, len(lo), mp, wmaps.size, op, R, q, 0, model, d),
                        lambda c, l, s, d0: L.ngd_run_windows_job_var_nj(h, lp, hp, len(lo), mp, wmaps.size, op, R, q, 0, model, c, l, s, d0)),
            "plain": (int(len(plo)), 1,
                      lambda d: L.ngd_run_windows_dist(h, plp, php, len(plo), 0, model, d),
                      lambda c, l, s, d0: L.ngd_run_windows_nj(h, plp, php, len(plo), 0, model, c, l, s, d0)),
        }
        for name in [s for s in args.shapes.split(",") if s]:
            n_set, n_mat, f_dist, f_nj = shapes[name]
            tot = n_set * n_mat
            dist = np.zeros((tot, n_pairs))  # (touched: no page faults inside the timed calls)
            child, length, status = np.zeros((tot, nb), dtype=np.int32), np.zeros((tot, nb)), np.zeros(tot, dtype=np.uint32)
            hchild, hlength, hstatus = np.zeros((tot, nb), dtype=np.int32), np.zeros((tot, nb)), np.zeros(tot, dtype=np.uint32)
            dist0 = np.zeros((n_set, n_pairs))

            def call_host():
                t0 = time.perf_counter()
                rc = f_dist(dist.ctypes.data_as(dp))
                assert rc == 0, L.ngd_last_error()
                t1 = time.perf_counter()
                rc = L.ngd_nj_host(dist.ctypes.data_as(dp), tot, n, hchild.ctypes.data_as(ip), hlength.ctypes.data_as(dp),
                                   hstatus.ctypes.data_as(u32p))
                assert rc == 0
                return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3

            def call_nj():
                t0 = time.perf_counter()
                rc = f_nj(child.ctypes.data_as(ip), length.ctypes.data_as(dp), status.ctypes.data_as(u32p), dist0.ctypes.data_as(dp))
                assert rc == 0, L.ngd_last_error()
                return (time.perf_counter() - t0) * 1e3, e.last_nj_ms()

            for _ in range(args.warmup):
                call_nj()
                assert f_dist(dist.ctypes.data_as(dp)) == 0, L.ngd_last_error()  # (the host form's device part, warmed up alike)
            t_nj, t_kern = [], []
            for _ in range(args.reps):
                w, k = call_nj()
                t_nj.append(w)
                t_kern.append(k)
            t_host, t_dist = [], []
            for _ in range(args.host_reps):
                w, d = call_host()
                t_host.append(w)
                t_dist.append(d)
            equal = int(sum(np.array_equal(child[k], hchild[k]) and np.array_equal(length[k].view(np.uint64), hlength[k].view(np.uint64))
                            for k in range(tot)))
            step = max(1, tot // 64)  # (the bipartitions of a sample: Python sets of up to 1000 leaves)
            sample = list(range(0, tot, step))
            same_tree = int(sum(status[k] == hstatus[k] and (not status[k] or splits(child[k], n) == splits(hchild[k], n))
                                for k in sample))
            sweep = None
            if args.wg_sweep and name == args.shapes.split(",")[0]:
                sweep = {256: [], 512: [], 1024: []}
                for _ in range(args.reps):
                    for wg in sweep:
                        os.environ["NGD_NJ_WG"] = str(wg)
                        sweep[wg].append(round(call_nj()[1], 3))
                os.environ["NGD_NJ_WG"] = str(wg_default)
                sweep = {str(k): {"kernel_ms_median": statistics.median(v), "kernel_ms_runs": v} for k, v in sweep.items()}
            # what the algorithm needs of the kernel: Q of every live pair at every join, 8 bytes of scratch read for each
            q_evals = int(status.sum()) * ((n + 1) * n * (n - 1) // 6 - 4)
            kern_s = statistics.median(t_kern) * 1e-3
            out = {"kernel_q_evaluations": q_evals, "kernel_scan_bytes": 8 * q_evals,
                   "kernel_scan_bytes_per_s": round(8 * q_evals / kern_s, 1) if kern_s else None,
                   "kernel_q_per_s": round(q_evals / kern_s, 1) if kern_s else None}
            out = {**{"shape": name, "n_ind": n, "n_sites": int(e.n_sites), "n_set": n_set, "n_mat_per_set": n_mat, "matrices": tot,
                   "block_size": q if n_mat > 1 else None, "evol_model": model, "warmup": args.warmup, "reps": args.reps,
                   "host_reps": args.host_reps, "host_threads": threads, "workgroup": wg_default,
                   "nj_ms_median": round(statistics.median(t_nj), 3), "nj_ms_runs": [round(x, 3) for x in t_nj],
                   "dist_then_host_nj_ms_median": round(statistics.median(t_host), 3), "dist_then_host_nj_ms_runs": [round(x, 3) for x in t_host],
                   "dist_part_ms_runs": [round(x, 3) for x in t_dist],
                   "nj_over_host": round(statistics.median(t_nj) / statistics.median(t_host), 4),
                   "kernel_device_ms_median": round(statistics.median(t_kern), 3), "kernel_device_ms_runs": [round(x, 3) for x in t_kern],
                   "host_bytes_to_host": tot * n_pairs * 16,
                   "nj_bytes_to_host": int(child.nbytes + length.nbytes + status.nbytes + n_set * n_pairs * 16),
                   "matrices_with_tree": int(status.sum()), "records_equal_to_host": equal,
                   "sampled_for_bipartitions": len(sample), "sampled_with_equal_bipartitions": same_tree, "wg_sweep": sweep}, **out}
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            del dist, child, length, status, hchild, hlength, hstatus, dist0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
