"""Windows along the genome on the device: one JSON line per (path, window shape, plan).

cfg 3's shape (1000 individuals x 1e6 sites, --indep_geno, synthetic data on the device): windows of 10 000 sites every
2 500 (397 windows) and of 100 sites every 100 (10 000 windows, their results left on the device in groups of 1 000);
then the EM path at 1000 x 1e5 (the table-driven kernel), windows of 10 000 sites every 2 500, both plans.  Each line holds
the windowed call's device time (ngd_last_windows().ms, summed over the groups: the best of --reps calls, every call's
time and their median beside it), a plain run() of the same engine in the same process, and the bytes of results.  Not
bench.py: that one measures the flagship workload and stays as it is.

    python tools/bench_windows.py [--n_ind 1000] [--n_sites 1000000] [--em_sites 100000] [--reps 2]
                                  [--skip_indep] [--skip_em] [--em_plans 2,1]
(--em_plans 1: an engine library without the EM form of the segment-slab plan, NGSDIST_AMD_LIB=...)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=1000000)
    ap.add_argument("--em_sites", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=2, help="timed calls per line (the best is reported)")
    ap.add_argument("--group", type=int, default=1000, help="windows per device call of the many-window shape")
    ap.add_argument("--skip_em", action="store_true")
    ap.add_argument("--skip_indep", action="store_true")
    ap.add_argument("--em_plans", default="2,1", help="plans of the EM leg (1 per window, 2 segment slab, 0 auto)")
    args = ap.parse_args()
    import torch

    import ngsdist_amd as N

    def plain_ms(e):
        e.run()
        best = None
        for _ in range(args.reps):
            e.run()
            t = e.timing()["ms_total"]
            best = t if best is None else min(best, t)
        return best

    def windowed(e, lo, hi, plan, group):
        e.set_option("win_plan", plan)
        n_pairs = e.n_pairs
        g = min(group, len(lo))
        d_sum = torch.empty((g, n_pairs), dtype=torch.float64, device="cuda")
        d_cnt = torch.empty((g, n_pairs), dtype=torch.int64, device="cuda")
        best = None
        runs = []
        for _ in range(args.reps):
            tot = {"ms": 0.0, "segments": 0, "batches": 0, "band_launches": 0, "windows_by_pass": 0, "fixup_pairs": 0,
                   "slab_bytes": 0}
            t0 = time.perf_counter()
            for w0 in range(0, len(lo), g):
                w1 = min(len(lo), w0 + g)
                e.run_windows(lo[w0:w1], hi[w0:w1], d_sum.data_ptr(), d_cnt.data_ptr())
                info = e.windows_info()
                for k in tot:
                    tot[k] = max(tot[k], info[k]) if k == "slab_bytes" else tot[k] + info[k]
            tot["wall_ms"] = (time.perf_counter() - t0) * 1e3
            runs.append(round(tot["ms"], 3))
            if best is None or tot["ms"] < best["ms"]:
                best = tot
        best["runs"] = runs
        return best

    def lines(e, path, shapes, plans):
        t_plain = plain_ms(e)
        for size, step, group in shapes:
            lo, hi = N.window_ranges(e.n_sites, size, step)
            for plan in plans:
                r = windowed(e, lo, hi, plan, group)
                out = {"path": path, "n_ind": e.n_ind, "n_sites": e.n_sites, "win_size": size, "win_step": step,
                       "n_win": int(len(lo)), "plan": {1: "per_window", 2: "segment_slab", 0: "auto"}[plan],
                       "device_ms": round(r["ms"], 3), "device_ms_runs": r["runs"],
                       "device_ms_median": sorted(r["runs"])[len(r["runs"]) // 2],
                       "wall_ms": round(r["wall_ms"], 3), "plain_run_ms": round(t_plain, 3),
                       "ratio_to_plain": round(r["ms"] / t_plain, 3) if t_plain else None,
                       "result_bytes": int(len(lo)) * e.n_pairs * 16, "segments": r["segments"], "batches": r["batches"],
                       "band_launches": r["band_launches"], "windows_by_pass": r["windows_by_pass"],
                       "fixup_pairs": r["fixup_pairs"], "slab_bytes": r["slab_bytes"]}
                print(json.dumps(out), flush=True)

    if not args.skip_indep:
        with N.Engine(args.n_ind, args.n_sites, indep_geno=True, kernel="mfma") as e:
            e.synth_fill(3, 0.0)
            lines(e, "indep_mfma_image_mode_%d" % e.image_mode()[0],
                  [(10000, 2500, args.group), (100, 100, args.group)], (2, 1))
    if not args.skip_em:
        with N.Engine(args.n_ind, args.em_sites, indep_geno=False, kernel="auto") as e:
            e.synth_fill(3, 0.0)
            lines(e, "em_auto", [(10000, 2500, args.group)], tuple(int(x) for x in args.em_plans.split(",")))


if __name__ == "__main__":
    main()
