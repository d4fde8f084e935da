#!/usr/bin/env python3
"""What NGD_OPT_EM_EXACT costs: the plain full-data pass of the table-driven EM kernel with the option off and on, on the
synthetic data set of bench.py's EM configuration (1000 individuals x 1e5 sites unless told otherwise), in ONE process
and alternating, so that the two share the clock and the machine's other load.  Prints one JSON line:

  ms_off / ms_on        median over the timed steps of the accumulation kernel alone (device events, ngd_last_timing)
  ms_total_off / _on    ... of the whole run call on the device (accumulation + reduction + counts)
  wall_on_ms            median host wall clock of the option-on call (includes the recheck: gather + host + patch)
  noted, changed, recheck_ms, passes   ngd_last_em_exact() of the last option-on step
  max_rel_diff          largest relative difference between the option-on and option-off sums (the pairs that were patched)
  pairs_patched         pairs whose sum differs at all

The option-off figure is the comparison: that instantiation of the kernel is the one the engine has always run
(cfg 4).

--job R --block_size B: the full data + R bootstrap replicates (block maps from Taus(seed + r)) as ONE ngd_run_job_dist call
(the job and its tail, evolutionary model 2: the emboot workload of bench.py), the option alternating 0 / 2 in one process:

  wall_off_ms / wall_on_ms   median host wall clock of the call (option 2: includes the recheck and the weighted patch)
  wall_off_all / wall_on_all every timed step: the spread the ratio on_over_off is to be read against
  ms_total_off / _on         ... of the engine's stream (ngd_last_timing)
  spill_off / spill_on       ngd_last_spill_timing() of the last step (the EM pass is ms_terms; zeros under another plan)
  plan_off_all / plan_on_all every timed step's plan: the spilled-terms plan's chunk count, 0 = per-block partials (the
                             engine buys the partials' slab only once the calls it would have saved add up to its allocation)
  terms_off_all / _on_all    every timed step's EM pass under the spilled-terms plan, ms (0 under per-block partials)
  noted, changed, recheck_ms, passes   ngd_last_em_exact() of the last option-2 step
  max_rel_diff, cells_patched          over every (matrix, pair) cell of the finished distances

--windows: the windowed EM shape of tools/bench_windows.py -- 37 windows of 10 000 sites every 2 500 at 1000 x 1e5, segment slab
(NGD_OPT_WIN_PLAN = 2), results in device memory -- with NGD_OPT_EM_EXACT 0 / 1 alternating (NGD_OPT_EM_EXACT_WIN on throughout:
it does nothing while the other is 0), and a plain-pass off / on pair in the same process to read the windowed ratio against:

  plain                      the plain leg's figures (ms_off, ms_on, on_over_off, their spread)
  accum_off_ms / accum_on_ms median of the slab's ONE accumulation launch (ngd_last_timing ms_accum): per pair-site the plain
                             noting form's work
  call_off_ms / call_on_ms   median of ngd_last_windows().ms: the call on the device, option on: + recheck and patch
  wall_off_ms / wall_on_ms   median host wall clock of the call
  accum_on_over_off, call_on_over_off, wall_on_over_off;  *_all: every timed step;  spread_*: (max - min) / median of them
  excess_over_plain          accum_on_over_off - plain.on_over_off, to be read against twice the spreads
  noted, changed, recheck_ms, passes   ngd_last_em_exact() of the last option-on call (the call's union)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def job(N, a, res):
    B = a.block_size
    maps = np.stack([N.Taus(a.seed + r).block_map(a.n_sites // B) for r in range(a.job)])
    res.update(job=a.job, block_size=B)
    med = statistics.median
    with N.Engine(a.n_ind, a.n_sites, indep_geno=False, kernel="em_table", pairwise_del=a.pairwise_del,
                  variant=a.variant) as e:
        e.synth_fill(a.seed, 0.05 if a.pairwise_del else 0.0)
        t = {k: {"total": [], "wall": [], "plan": [], "terms": []} for k in (0, 2)}
        out = {0: np.empty((a.job + 1, e.n_pairs)), 2: np.empty((a.job + 1, e.n_pairs))}
        spill, info = {}, None
        for step in range(a.warmup + a.steps):
            for on in (0, 2):  # alternating: both see the same clock and the same neighbours
                e.set_option("em_exact", on)
                w0 = time.perf_counter()
                e.run_job_dist(maps, B, 2, out=out[on])
                wall = (time.perf_counter() - w0) * 1e3
                if step >= a.warmup:
                    t[on]["total"].append(e.timing()["ms_total"])
                    t[on]["wall"].append(wall)
                spill[on] = e.spill_timing()
                if step >= a.warmup:
                    t[on]["plan"].append(int(spill[on]["chunks"]))
                    t[on]["terms"].append(spill[on]["ms_terms"])
                if on:
                    info = e.last_em_exact()
        res["shader_clock_mhz"] = e.shader_clock_mhz()
    res.update(wall_off_ms=med(t[0]["wall"]), wall_on_ms=med(t[2]["wall"]), ms_total_off=med(t[0]["total"]),
               ms_total_on=med(t[2]["total"]), wall_off_all=t[0]["wall"], wall_on_all=t[2]["wall"], plan_off_all=t[0]["plan"],
               plan_on_all=t[2]["plan"], terms_off_all=t[0]["terms"], terms_on_all=t[2]["terms"], spill_off=spill[0],
               spill_on=spill[2])
    res["on_over_off"] = res["wall_on_ms"] / res["wall_off_ms"]
    res.update(noted=int(info["noted"]), changed=int(info["changed"]), recheck_ms=info["ms"], passes=int(info["passes"]))
    with np.errstate(all="ignore"):
        d = np.abs(out[2] - out[0])
        res["cells_patched"] = int(np.count_nonzero(d > 0))
        res["max_rel_diff"] = float(np.nanmax(d / np.abs(out[0])))
    print(json.dumps(res))


def plain(e, a):
    """the plain full-data pass, option 0 / 1 alternating: accumulation kernel alone, the run call, host wall clock"""
    t = {0: {"accum": [], "total": [], "wall": []}, 1: {"accum": [], "total": [], "wall": []}}
    sums, info = {}, None
    for step in range(a.warmup + a.steps):
        for on in (0, 1):  # alternating: both see the same clock and the same neighbours
            e.set_option("em_exact", on)
            w0 = time.perf_counter()
            s, c = e.run()
            wall = (time.perf_counter() - w0) * 1e3
            if step >= a.warmup:
                tm = e.timing()
                t[on]["accum"].append(tm["ms_accum"])
                t[on]["total"].append(tm["ms_total"])
                t[on]["wall"].append(wall)
            sums[on] = s
            if on:
                info = e.last_em_exact()
    e.set_option("em_exact", 0)
    return t, sums, info


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def windows(N, a, res):
    import torch
    med = statistics.median
    with N.Engine(a.n_ind, a.n_sites, indep_geno=False, kernel="em_table", pairwise_del=a.pairwise_del,
                  variant=a.variant) as e:
        e.synth_fill(a.seed, 0.05 if a.pairwise_del else 0.0)
        tp, _, _ = plain(e, a)
        res["plain"] = dict(ms_off=med(tp[0]["accum"]), ms_on=med(tp[1]["accum"]), ms_off_all=tp[0]["accum"],
                            ms_on_all=tp[1]["accum"], on_over_off=med(tp[1]["accum"]) / med(tp[0]["accum"]),
                            spread_off=spread(tp[0]["accum"]), spread_on=spread(tp[1]["accum"]),
                            wall_off_ms=med(tp[0]["wall"]), wall_on_ms=med(tp[1]["wall"]))
        lo, hi = N.window_ranges(a.n_sites, a.win_size, a.win_step)
        res.update(win_size=a.win_size, win_step=a.win_step, n_win=int(len(lo)))
        e.set_option("win_plan", 2)
        e.set_option("em_exact_win", 1)
        d_sum = {on: torch.empty((len(lo), e.n_pairs), dtype=torch.float64, device="cuda") for on in (0, 1)}
        d_cnt = torch.empty((len(lo), e.n_pairs), dtype=torch.int64, device="cuda")
        t = {on: {"accum": [], "call": [], "wall": []} for on in (0, 1)}
        info = wi = None
        for step in range(a.warmup + a.steps):
            for on in (0, 1):
                e.set_option("em_exact", on)
                w0 = time.perf_counter()
                e.run_windows(lo, hi, d_sum[on].data_ptr(), d_cnt.data_ptr())
                wall = (time.perf_counter() - w0) * 1e3
                wi = e.windows_info()
                if step >= a.warmup:
                    t[on]["accum"].append(e.timing()["ms_accum"])
                    t[on]["call"].append(wi["ms"])
                    t[on]["wall"].append(wall)
                if on:
                    info = e.last_em_exact()
        torch.cuda.synchronize()
        res["shader_clock_mhz"] = e.shader_clock_mhz()
        res.update(segments=int(wi["segments"]), batches=int(wi["batches"]), slab_bytes=int(wi["slab_bytes"]))
        d = (d_sum[1] - d_sum[0]).abs()
        res["cells_patched"] = int(torch.count_nonzero(d).item())
        res["max_rel_diff"] = float(torch.nan_to_num(d / d_sum[0].abs(), nan=0.0).max().item())
    for k in ("accum", "call", "wall"):
        res["%s_off_ms" % k], res["%s_on_ms" % k] = med(t[0][k]), med(t[1][k])
        res["%s_off_all" % k], res["%s_on_all" % k] = t[0][k], t[1][k]
        res["%s_on_over_off" % k] = med(t[1][k]) / med(t[0][k])
        res["spread_%s_off" % k], res["spread_%s_on" % k] = spread(t[0][k]), spread(t[1][k])
    res["excess_over_plain"] = res["accum_on_over_off"] - res["plain"]["on_over_off"]
    res.update(noted=int(info["noted"]), changed=int(info["changed"]), recheck_ms=info["ms"], passes=int(info["passes"]))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ind", type=int, default=1000)
    ap.add_argument("--n_sites", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pairwise_del", action="store_true")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--job", type=int, default=0, help="R: time the full data + R replicates (option 0 / 2) instead of the plain pass")
    ap.add_argument("--block_size", type=int, default=1)
    ap.add_argument("--windows", action="store_true", help="time the windowed call (option 0 / 1) beside a plain-pass pair")
    ap.add_argument("--win_size", type=int, default=10000)
    ap.add_argument("--win_step", type=int, default=2500)
    a = ap.parse_args()
    import ngsdist_amd as N
    if N.device_count() < 1:
        sys.exit("bench_em_exact: no GPU (nothing is measured without one)")
    res = {"tool": "bench_em_exact", "n_ind": a.n_ind, "n_sites": a.n_sites, "steps": a.steps, "warmup": a.warmup,
           "pairwise_del": bool(a.pairwise_del), "variant": a.variant}
    if a.job:
        return job(N, a, res)
    if a.windows:
        return windows(N, a, res)
    with N.Engine(a.n_ind, a.n_sites, indep_geno=False, kernel="em_table", pairwise_del=a.pairwise_del,
                  variant=a.variant) as e:
        e.synth_fill(a.seed, 0.05 if a.pairwise_del else 0.0)
        t, sums, info = plain(e, a)
        res["shader_clock_mhz"] = e.shader_clock_mhz()
        res["pair_sites"] = e.timing()["pair_sites"]
    med = statistics.median
    res.update(ms_off=med(t[0]["accum"]), ms_on=med(t[1]["accum"]), ms_total_off=med(t[0]["total"]),
               ms_total_on=med(t[1]["total"]), wall_off_ms=med(t[0]["wall"]), wall_on_ms=med(t[1]["wall"]),
               ms_off_all=t[0]["accum"], ms_on_all=t[1]["accum"])
    res["on_over_off"] = res["ms_on"] / res["ms_off"]
    res.update(noted=int(info["noted"]), changed=int(info["changed"]), recheck_ms=info["ms"], passes=int(info["passes"]))
    d = np.abs(sums[1] - sums[0])
    res["pairs_patched"] = int(np.count_nonzero(d))
    with np.errstate(all="ignore"):
        res["max_rel_diff"] = float(np.nanmax(d / np.abs(sums[0]))) if d.size else 0.0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
