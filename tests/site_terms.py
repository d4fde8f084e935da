"""A high-precision reference for every weighted plan of the EM path (a plain module, no tests).

On the EM path the term c(pair, site) that gen_dist() adds (ngsDist.cpp:351-353 after em2()) does not depend on the
replicate, only its weight does.  So the sum of any matrix of a job is linear in per-site terms,
    sum[r][pair] = SUM_s W[r][s] * c[s][pair],
and the oracle on one-site slices gives those terms once for all matrices.  combine() adds them up in extended
precision; counts come from the same weights in integers.
"""
import math

import numpy as np

from oracle import oracle as O

LONG_OK = np.finfo(np.longdouble).eps < 1e-18  # x87 extended or better; else math.fsum per cell


def site_terms(p, pairwise_del, indep_geno, score=None):
    """-> (terms float64[n_sites][n_pairs], valid uint64[n_sites][n_pairs]): what one site adds to a pair's sum and to
    its count, from O.all_pairs on each one-site slice p[:, s:s+1]"""
    n_ind, n_sites, _ = p.shape
    terms = np.empty((n_sites, O.n_pairs(n_ind)), dtype=np.float64)
    valid = np.empty((n_sites, O.n_pairs(n_ind)), dtype=np.uint64)
    for s in range(n_sites):
        terms[s], valid[s] = O.all_pairs(p[:, s:s + 1], score=score, pairwise_del=pairwise_del, indep_geno=indep_geno)
    return terms, valid


def job_weights(n_sites, block_size, maps=None, lead=False, mult=None):
    """W int64[n_mat][n_sites]: the lead matrix takes 1 on every site; a replicate takes mult[r][s // B] for s < n_eff
    (n_eff = n_blocks * B), else 0.  maps: block maps [n_rep][n_blocks] (their multiplicities are counted here)."""
    if mult is None:
        maps = np.asarray(maps, dtype=np.int64)
        mult = np.stack([np.bincount(m, minlength=maps.shape[1]) for m in maps]) if len(maps) else np.zeros((0, 0), np.int64)
    mult = np.asarray(mult, dtype=np.int64)
    n_rep, n_blocks = mult.shape if mult.size else (0, 0)
    n_eff = n_blocks * block_size
    assert n_eff <= n_sites
    W = np.zeros((n_rep + (1 if lead else 0), n_sites), dtype=np.int64)
    if lead:
        W[0] = 1
    if n_rep:
        W[1 if lead else 0:, :n_eff] = np.repeat(mult, block_size, axis=1)
    return W


def combine(W, terms):
    """sum_s W[r, s] * terms[s] for every matrix r, accumulated in np.longdouble (math.fsum per cell where long double is
    no wider than double), rounded to float64 once.  A site of weight 0 adds nothing (not 0 x NaN); a term that is not
    finite makes the cell NaN in exactly the matrices that weight its site."""
    W = np.asarray(W, dtype=np.int64)
    bad = ~np.isfinite(terms)
    t = np.where(bad, 0.0, terms)
    if LONG_OK:
        out = (W.astype(np.longdouble) @ t.astype(np.longdouble)).astype(np.float64)
    else:
        out = np.empty((W.shape[0], t.shape[1]), dtype=np.float64)
        for r in range(W.shape[0]):
            live = np.nonzero(W[r])[0]
            for k in range(t.shape[1]):
                out[r, k] = math.fsum(float(W[r, s]) * t[s, k] for s in live)  # (products of a small integer: 1 ulp each)
    poisoned = (W != 0).astype(np.int64) @ bad.astype(np.int64) > 0
    out[poisoned] = np.nan
    return out


def combine_counts(W, valid, pairwise_del):
    """the integer counts of every matrix: sum_s W[r, s] * valid[s] with --pairwise_del, else sum_s W[r, s] in every cell"""
    W = np.asarray(W, dtype=np.int64)
    if pairwise_del:
        return (W @ valid.astype(np.int64)).astype(np.uint64)
    return np.repeat(W.sum(axis=1)[:, None], valid.shape[1], axis=1).astype(np.uint64)
