"""Bootstrap replicates inside windows on the device: one JSON line per (path, leg).

1000 individuals x 1e5 sites (synthetic data on the device), windows of 10 000 sites every 2 500, blocks of 100 sites, 100
replicates -- on the --indep_geno path (the default engine: one image above 384 padded individuals) and on the EM path.  Legs:
  unit_slab   Engine.run_windows_job under NGD_OPT_WIN_PLAN = 2, results left on the device;
  per_window  the same call under NGD_OPT_WIN_PLAN = 1;
  baseline    what a caller did before the call existed: one Engine.run_batch(mult=...) per window, the window's full-data
              vector and its replicates as multiplicity vectors over blocks of gcd(lo, q, hi) sites from the engine's site
              0.  It uses only calls that older engine libraries have, so this file runs unchanged in a checkout without
              run_windows_job: there the two other legs are reported as absent and the baseline's figure is the comparison.
Each line holds the best device time of --reps calls (every call's time beside it), the wall time of that call, a plain run()
of the same engine in the same process, and the bytes of results.  Not bench.py: that one measures the flagship workload.

    python tools/bench_windows_boot.py [--n_ind 1000] [--n_sites 100000] [--win_size 10000] [--win_step 2500]
                                       [--block 100] [--n_rep 100] [--reps 2] [--skip_indep] [--skip_em] [--legs ...]

--bp: windows in base pairs, of unequal length (Engine.run_windows_job_var).  Synthetic positions -- gaps of 1 .. 39 bp
between sites, every 50th stretch of 100 sites twelve times sparser -- and windows of --win_bp every --win_bp_step (20 000
every 4 000: about 1000 sites, 5 x overlap), blocks of 10 and of 100 sites.  The results of all windows do not fit a device
(500 windows x 101 matrices x 8 MB at 1000 individuals), so the windows go through in groups of --group whose results share
one buffer; --max_windows takes the first so many.  Legs, one JSON line each, the MEDIAN device time of --reps calls after
one warm-up call:
  unit_slab   run_windows_job_var under NGD_OPT_WIN_PLAN = 2;      per_window  the same under NGD_OPT_WIN_PLAN = 1;
  auto        the same under NGD_OPT_WIN_PLAN = 0 (which plan it took: windows_by_pass);
  baseline    the only route before the call existed: one run_windows_job per window, in a Python loop (auto plan).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=100000)
    ap.add_argument("--win_size", type=int, default=10000)
    ap.add_argument("--win_step", type=int, default=2500)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--n_rep", type=int, default=100)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2, help="timed calls per line (the best is reported)")
    ap.add_argument("--skip_em", action="store_true")
    ap.add_argument("--skip_indep", action="store_true")
    ap.add_argument("--legs", default="unit_slab,per_window,baseline")
    ap.add_argument("--bp", action="store_true", help="windows in base pairs through run_windows_job_var")
    ap.add_argument("--win_bp", type=int, default=20000)
    ap.add_argument("--win_bp_step", type=int, default=4000)
    ap.add_argument("--blocks", default="10,100", help="--bp: block sizes, one set of lines each")
    ap.add_argument("--group", type=int, default=16, help="--bp: windows per call (their results share one device buffer)")
    ap.add_argument("--max_windows", type=int, default=0, help="--bp: only the first so many windows (0: all)")
    args = ap.parse_args()
    if args.bp:
        return main_bp(args)
    import numpy as np
    import torch

    import ngsdist_amd as N

    q, R, W = args.block, args.n_rep, args.win_size
    n_blocks = W // q
    t = N.Taus(args.seed)
    maps = np.stack([t.block_map(n_blocks) for _ in range(R)])
    mult = np.zeros((R, n_blocks), dtype=np.uint32)
    for r in range(R):
        np.add.at(mult[r], maps[r].astype(np.int64), 1)

    def plain_ms(e):
        e.run()
        best = None
        for _ in range(args.reps):
            e.run()
            ms = e.timing()["ms_total"]
            best = ms if best is None else min(best, ms)
        return best

    def job(e, lo, hi, plan, d_sum, d_cnt):
        e.set_option("win_plan", plan)
        e.run_windows_job(lo, hi, maps, q, d_sum.data_ptr(), d_cnt.data_ptr())
        info = e.windows_info()
        fx = e.fixup()
        return info["ms"], {k: info[k] for k in ("segments", "batches", "band_launches", "windows_by_pass", "fixup_pairs",
                                                 "slab_bytes")} | {"fixup_ms": round(fx["ms"], 3)}

    def baseline(e, lo, hi, d_sum, d_cnt):
        ms = 0.0
        per = (R + 1) * e.n_pairs * 8
        for w, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
            B = math.gcd(math.gcd(a, q), b)
            n_eb, first, k = b // B, a // B, q // B
            m = np.zeros((R + 1, n_eb), dtype=np.uint32)
            m[0, first:] = 1
            m[1:, first:first + n_blocks * k] = np.repeat(mult, k, axis=1)
            e.run_batch(mult=m, block_size=B, d_sum_ptr=d_sum.data_ptr() + w * per, d_cnt_ptr=d_cnt.data_ptr() + w * per)
            ms += e.timing()["ms_total"] + e.fixup()["ms"]
        return ms, {}

    def lines(e, path):
        t_plain = plain_ms(e)
        lo, hi = N.window_ranges(e.n_sites, W, args.win_step)
        d_sum = torch.empty((len(lo), R + 1, e.n_pairs), dtype=torch.float64, device="cuda")
        d_cnt = torch.empty((len(lo), R + 1, e.n_pairs), dtype=torch.int64, device="cuda")
        for leg in args.legs.split(","):
            out = {"path": path, "leg": leg, "n_ind": e.n_ind, "n_sites": e.n_sites, "win_size": W, "win_step": args.win_step,
                   "n_win": int(len(lo)), "block": q, "n_rep": R, "plain_run_ms": round(t_plain, 3),
                   "result_bytes": int(len(lo)) * (R + 1) * e.n_pairs * 16}
            if leg != "baseline" and not hasattr(e, "run_windows_job"):
                out["absent"] = True
                print(json.dumps(out), flush=True)
                continue
            runs, best, best_wall, extra = [], None, None, {}
            for _ in range(args.reps):
                e.drop_caches()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if leg == "baseline":
                    ms, x = baseline(e, lo, hi, d_sum, d_cnt)
                else:
                    ms, x = job(e, lo, hi, 2 if leg == "unit_slab" else 1, d_sum, d_cnt)
                wall = (time.perf_counter() - t0) * 1e3
                runs.append(round(ms, 3))
                if best is None or ms < best:
                    best, best_wall, extra = ms, wall, x
            out.update({"device_ms": round(best, 3), "device_ms_runs": runs, "wall_ms": round(best_wall, 3),
                        "ratio_to_plain": round(best / t_plain, 3) if t_plain else None})
            out.update(extra)
            print(json.dumps(out), flush=True)

    if not args.skip_indep:
        with N.Engine(args.n_ind, args.n_sites, indep_geno=True, kernel="mfma") as e:
            e.synth_fill(3, 0.0)
            lines(e, "indep_mfma_image_mode_%d" % e.image_mode()[0])
    if not args.skip_em:
        with N.Engine(args.n_ind, args.n_sites, indep_geno=False, kernel="auto") as e:
            e.synth_fill(3, 0.0)
            lines(e, "em_auto")


def main_bp(args):
    import statistics

    import numpy as np
    import torch

    import ngsdist_amd as N

    R = args.n_rep
    rng = np.random.default_rng(3)
    gaps = rng.integers(1, 40, args.n_sites)
    sparse = (np.arange(args.n_sites) // 100) % 50 == 49
    gaps[sparse] *= 12
    pos = np.cumsum(gaps)
    lo, hi, _ = N.window_ranges_bp(pos, args.win_bp, args.win_bp_step)
    if args.max_windows:
        lo, hi = lo[:args.max_windows], hi[:args.max_windows]
    legs = args.legs.split(",") if args.legs != "unit_slab,per_window,baseline" else ["unit_slab", "per_window", "auto", "baseline"]

    def one_call(e, leg, q, maps, off, d_sum, d_cnt):
        """all windows, group by group -> (device ms, what the plans did)"""
        ms, took = 0.0, {"segments": 0, "batches": 0, "windows_by_pass": 0, "fixup_pairs": 0}
        e.set_option("win_plan", {"unit_slab": 2, "per_window": 1}.get(leg, 0))
        for g0 in range(0, len(lo), args.group):
            l, h, o = lo[g0:g0 + args.group], hi[g0:g0 + args.group], off[g0:g0 + args.group]
            if leg != "baseline":
                e.run_windows_job_var(l, h, maps, o, q, d_sum.data_ptr(), d_cnt.data_ptr(), n_rep=R)
                info = e.windows_info()
                ms += info["ms"]
                for k in took:
                    took[k] += info[k]
                continue
            per = (R + 1) * e.n_pairs * 8
            for w in range(len(l)):
                nb = int(h[w] - l[w]) // q
                if not nb:  # (the old call refuses a window without a block: its matrix 0 alone)
                    e.run_windows(l[w:w + 1], h[w:w + 1], d_sum.data_ptr() + w * per, d_cnt.data_ptr() + w * per)
                else:
                    m = maps[int(o[w]):int(o[w]) + R * nb].reshape(R, nb)
                    e.run_windows_job(l[w:w + 1], h[w:w + 1], m, q, d_sum.data_ptr() + w * per, d_cnt.data_ptr() + w * per)
                info = e.windows_info()
                ms += info["ms"]
                took["windows_by_pass"] += info["windows_by_pass"]
                took["batches"] += info["batches"]
        return ms, took

    def lines(e, path):
        d_sum = torch.empty((args.group, R + 1, e.n_pairs), dtype=torch.float64, device="cuda")
        d_cnt = torch.empty((args.group, R + 1, e.n_pairs), dtype=torch.int64, device="cuda")
        L = (hi - lo).astype(np.int64)
        for q in [int(x) for x in args.blocks.split(",")]:
            maps, off = N.window_boot_maps(args.seed, lo, hi, R, q)
            for leg in legs:
                one_call(e, leg, q, maps, off, d_sum, d_cnt)  # warm-up: allocations, code objects
                runs = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ms, took = one_call(e, leg, q, maps, off, d_sum, d_cnt)
                    torch.cuda.synchronize()
                    runs.append((ms, (time.perf_counter() - t0) * 1e3))
                out = {"path": path, "leg": leg, "n_ind": e.n_ind, "n_sites": e.n_sites, "win_bp": args.win_bp,
                       "win_bp_step": args.win_bp_step, "n_win": int(len(lo)), "sites_per_window_min_median_max":
                       [int(L.min()), int(np.median(L)), int(L.max())], "distinct_lengths": int(len(set(L.tolist()))), "block": q,
                       "n_rep": R, "group": args.group, "device_ms_median": round(statistics.median(r[0] for r in runs), 3),
                       "device_ms_runs": [round(r[0], 3) for r in runs], "wall_ms_median": round(statistics.median(r[1] for r in runs), 3)}
                out.update(took)
                print(json.dumps(out), flush=True)

    if not args.skip_indep:
        with N.Engine(args.n_ind, args.n_sites, indep_geno=True, kernel="mfma") as e:
            e.synth_fill(3, 0.0)
            lines(e, "indep_mfma_image_mode_%d" % e.image_mode()[0])
    if not args.skip_em:
        with N.Engine(args.n_ind, args.n_sites, indep_geno=False, kernel="auto") as e:
            e.synth_fill(3, 0.0)
            lines(e, "em_auto")


if __name__ == "__main__":
    main()
