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
    args = ap.parse_args()
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


if __name__ == "__main__":
    main()
