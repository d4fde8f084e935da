#!/usr/bin/env python3
"""What create_slices (ngsdist_amd/csrc/engine_create.hip) plans for the plain pass of a one-image engine in congruent
coordinates, on the host: the slice count n_ks and the length of a slice of the pass that leaves the unit-sum coordinate out
(skip_per_slice list entries = 2 per period of four sites), for the largest data set of each n_ind that fits the device.
Needs no device: the arithmetic of create_jobs / create_slices for engines above 384 padded individuals (form 0, the
engine's own choice of slices, 256 CUs in 8 XCDs) and the sizes create_images allocates.

  python tools/unit_skip_slices.py [--hbm-gb 288]"""
import argparse
import math


def n_wg(n_ind):
    """workgroups per slice: an off-diagonal 128-tile is one, the live 64 x 64 blocks of the diagonal tiles go four to one"""
    n_t, n_igv = (n_ind + 127) // 128, (n_ind + 15) // 16
    diag = 0
    for t in range(n_t):
        r0 = 8 * t
        diag += sum(1 for r, c in ((r0, r0), (r0, r0 + 4), (r0 + 4, r0 + 4)) if r < n_igv and c < n_igv)
    return n_t * (n_t - 1) // 2 + (diag + 3) // 4


def plan(n_ind, n_sites, n_slices=0, cus=256):
    n_sites_pad = (n_sites + 15) // 16 * 16
    n_kg = 3 * n_sites_pad // 4
    n_kgskip = n_kg // 3 * 2
    wg = max(1, n_wg(n_ind))
    ks = (8192 + wg - 1) // wg
    max_ks = max(8, n_kg // 128)
    ks = max(8, (min(ks, max_ks) + 7) // 8 * 8)
    slots = cus // 8 * 3
    pairs = n_ind * (n_ind - 1) // 2
    accum_s = 6.0 * pairs * n_sites / (0.8 * 78.6e12)
    per_slice_s = 8.0 * pairs / 5e12
    best, best_ks = 1e30, ks
    for c in range(max(8, ks // 3 // 8 * 8), min(max_ks, ks * 115 // 100) + 1, 8):
        rounds = wg * (c // 8) / slots
        waste = math.ceil(rounds - 1e-9) / rounds + c * per_slice_s / max(accum_s, 1e-9)
        if waste < best:
            best, best_ks = waste, c
    ks = best_ks
    if n_slices:
        ks = min(n_slices, max_ks)
    ks = max(8, (ks + 7) // 8 * 8)
    skip_per_slice = ((n_kgskip + ks - 1) // ks + 3) // 4 * 4
    return ks, skip_per_slice, 2 * skip_per_slice


def device_bytes(n_ind, n_sites, ks):
    """the image, the side array of min(p0, p2), the per-index weights, the slab and the results"""
    n_pad = (n_ind + 127) // 128 * 128
    n_sites_pad = (n_sites + 15) // 16 * 16
    n_kg = 3 * n_sites_pad // 4
    pairs = n_ind * (n_ind - 1) // 2
    return ((n_kg + 8) * (n_pad // 16) * 64 * 8 + n_sites * n_ind * 8 + (n_sites_pad + 32) * 8 + 2 * 4 * (n_kg + 8) * 8
            + 4 * (n_kgskip_of(n_kg) + 16) + ks * n_pad * n_pad * 8 + 16 * pairs)


def n_kgskip_of(n_kg):
    return n_kg // 3 * 2


def largest(n_ind, hbm):
    lo, hi = 16, 1 << 36
    while hi - lo > 16:
        mid = (lo + hi) // 2 // 16 * 16
        if device_bytes(n_ind, mid, plan(n_ind, mid)[0]) <= hbm:
            lo = mid
        else:
            hi = mid
    return lo


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hbm-gb", type=float, default=288.0)
    a = ap.parse_args()
    print("cfg 3 (1000 x 1 000 000): n_ks %d, skip_per_slice %d list entries = %d sites" % plan(1000, 1_000_000))
    print("largest data set that fits %.0f GB, by n_ind:" % a.hbm_gb)
    print("%8s %14s %6s %16s %16s" % ("n_ind", "n_sites", "n_ks", "skip_per_slice", "sites per slice"))
    for n_ind in (400, 600, 1000, 2000, 4000, 8000, 16000, 32000):
        n_sites = largest(n_ind, a.hbm_gb * 1e9)
        ks, sps, sites = plan(n_ind, n_sites)
        print("%8d %14d %6d %16d %16d" % (n_ind, n_sites, ks, sps, sites))
