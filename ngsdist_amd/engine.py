"""Host-side handle on the MI355X engine (ctypes over include/ngsdist_amd.h).

The reference is a compiled C++ program, so the product's host is the C++
driver under ngsdist_amd/csrc/host/ (same command line as ngsDist); this module
is the thin Python door the tests and bench.py use.  Names follow the
reference: gen_dist / evol_model / pairwise_del / indep_geno / tot_sites /
boot_block_size (ngsDist.hpp:11-44).
"""
import ctypes as C

import numpy as np

from . import _lib

KERNELS = {"auto": 0, "stream": 1, "mfma": 2, "em_faithful": 3, "em_fast": 4, "em_table": 5}
# NGD_OPT_* of include/ngsdist_amd.h
OPTIONS = {"boot_partials": 1, "boot_max_bytes": 2, "boot_wg": 3, "boot_unaligned": 4, "em_batch": 5,
           "em_spill": 6, "em_spill_bytes": 7, "single_image_bytes": 8, "fixup_work": 9, "stage_piece_mib": 10,
           "stage_ring": 11, "eager_full": 12, "win_plan": 13, "win_max_bytes": 14, "em_exact": 15, "em_exact_cap": 16,
           "unit_skip": 17, "em_exact_win": 18, "nj_max_bytes": 19, "mds_max_bytes": 20, "win_cmp_max_bytes": 21,
           "debug_forge_job": 100}
# ngd_em_exact_entry
EM_EXACT_ENTRY = np.dtype([("i1", np.uint32), ("i2", np.uint32), ("site", np.uint64), ("t_dev", np.uint32),
                           ("t_ref", np.uint32), ("c_dev", np.float64), ("c_ref", np.float64)], align=True)

# parse_args.cpp:25-27
DEFAULT_SCORE = (0.0, 0.5, 1.0, 0.5, 0.0, 0.5, 1.0, 0.5, 0.0)


class NgdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ngsdist_amd error %d: %s" % (code, msg))
        self.code = code


def _check(rc):
    if rc != 0:
        raise NgdError(rc, _lib.load().ngd_last_error().decode(errors="replace"))


def device_count():
    return _lib.load().ngd_device_count()


def n_pairs(n_ind):
    return n_ind * (n_ind - 1) // 2


def score_matrix(avg_nuc_dist=False):
    s = list(DEFAULT_SCORE)
    if avg_nuc_dist:  # --avg_nuc_dist, parse_args.cpp:134-137
        s[4] = 0.5
    return s


class Engine:
    """One resident data set on one GPU; `run()` = one replicate's worth of
    gen_dist() over every pair this engine's shard owns."""

    def __init__(self, n_ind, n_sites, score=None, pairwise_del=False, indep_geno=True, kernel="auto",
                 device=-1, shard_rank=0, shard_world=1, variant=0, n_slices=0, wg_target=0, exact_shapes=0,
                 single_image=0, second_image_bytes=0):
        self._L = _lib.load()
        self._h = C.c_void_p()
        cfg = _lib.NgdConfig()
        cfg.n_ind, cfg.n_sites = int(n_ind), int(n_sites)
        sc = DEFAULT_SCORE if score is None else [float(x) for x in np.asarray(score).reshape(9)]
        for k in range(9):
            cfg.score[k] = sc[k]
        cfg.pairwise_del, cfg.indep_geno = int(bool(pairwise_del)), int(bool(indep_geno))
        cfg.device, cfg.kernel = int(device), KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        cfg.shard_rank, cfg.shard_world = int(shard_rank), int(shard_world)
        # launch geometry, 0 = the engine's defaults (ngd_config)
        cfg.variant, cfg.n_slices, cfg.wg_target, cfg.exact_shapes = int(variant), int(n_slices), int(wg_target), int(exact_shapes)
        # MFMA kernel, operand images: 0 = the engine's choice, 1 / True: one + the other formed per launch, 2: one in
        # congruent coordinates (+ the fix-up pass of nearly identical pairs), 3: two
        cfg.single_image = int(single_image)
        cfg.second_image_mib = int(second_image_bytes) >> 20  # ... except this much of it, kept resident all the same
        self.n_ind, self.n_sites = int(n_ind), int(n_sites)
        self.n_pairs = n_pairs(self.n_ind)
        _check(self._L.ngd_create(C.byref(cfg), C.byref(self._h)))

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.ngd_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- input --------------------------------------------------------------
    def upload_ind_major(self, p):
        """p[n_ind][n_sites][3]: in_geno_lkl as gen_dist reads it (normal space)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert p.shape == (self.n_ind, self.n_sites, 3), p.shape
        _check(self._L.ngd_upload_ind_major(self._h, p.ctypes.data_as(C.POINTER(C.c_double))))
        return self

    def upload_sites(self, p, s0=0):
        """p[n][n_ind][3]: a run of sites in the binary file's order."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert p.ndim == 3 and p.shape[1:] == (self.n_ind, 3), p.shape
        _check(self._L.ngd_upload_sites(self._h, p.ctypes.data_as(C.POINTER(C.c_double)), int(s0), p.shape[0]))
        return self

    def upload_raw_sites(self, raw, s0=0, in_logscale=False, call_geno=False, N_thresh=0.0, call_thresh=0.0):
        """raw[n][n_ind][3]: doubles as stored in the binary GL file; prepared on the device."""
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        assert raw.ndim == 3 and raw.shape[1:] == (self.n_ind, 3), raw.shape
        pr = _lib.NgdPrep(int(in_logscale), int(call_geno), float(N_thresh), float(call_thresh))
        _check(self._L.ngd_upload_raw_sites(self._h, raw.ctypes.data_as(C.POINTER(C.c_double)), int(s0),
                                            raw.shape[0], C.byref(pr)))
        return self

    def commit(self):
        _check(self._L.ngd_commit(self._h))
        return self

    def synth_fill(self, seed, miss_frac=0.0, site0=0):
        """synthetic data set; site0 = position of this engine's first site in the whole set (site sharding)"""
        _check(self._L.ngd_synth_fill_range(self._h, int(seed), float(miss_frac), int(site0)))
        return self

    # -- the hot path ---------------------------------------------------------
    def _map_args(self, block_map, block_size):
        if block_map is None:
            return None, 0, 0, None
        bm = np.ascontiguousarray(block_map, dtype=np.uint64)
        return bm.ctypes.data_as(C.POINTER(C.c_uint64)), bm.size, int(block_size), bm

    def run(self, block_map=None, block_size=1):
        """-> (sum float64[n_pairs], cnt uint64[n_pairs]) in the reference's pair order."""
        ptr, nb, bs, keep = self._map_args(block_map, block_size)
        s = np.empty(self.n_pairs, dtype=np.float64)
        c = np.empty(self.n_pairs, dtype=np.uint64)
        _check(self._L.ngd_run(self._h, ptr, nb, bs, s.ctypes.data_as(C.POINTER(C.c_double)),
                               c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_mult(self, mult, block_size, d_sum_ptr=None, d_cnt_ptr=None):
        """one replicate from the multiplicity of each of this engine's blocks (site sharding)"""
        m = np.ascontiguousarray(mult, dtype=np.uint32)
        mp = m.ctypes.data_as(C.POINTER(C.c_uint32))
        if d_sum_ptr is not None:
            _check(self._L.ngd_run_mult_device(self._h, mp, m.size, int(block_size), C.c_void_p(d_sum_ptr),
                                               C.c_void_p(d_cnt_ptr)))
            return None
        s = np.empty(self.n_pairs, dtype=np.float64)
        c = np.empty(self.n_pairs, dtype=np.uint64)
        _check(self._L.ngd_run_mult(self._h, mp, m.size, int(block_size), s.ctypes.data_as(C.POINTER(C.c_double)),
                                    c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_batch(self, block_maps=None, block_size=1, mult=None, d_sum_ptr=None, d_cnt_ptr=None):
        """n_rep bootstrap replicates in one call (ngd_run_batch / ngd_run_mult_batch): block_maps or mult is
        [n_rep][n_blocks]; returns (sum, cnt) of shape [n_rep][n_pairs], or writes them to device buffers."""
        if (block_maps is None) == (mult is None):
            raise ValueError("give block_maps or mult")
        if mult is None:
            a = np.ascontiguousarray(block_maps, dtype=np.uint64)
            ap = a.ctypes.data_as(C.POINTER(C.c_uint64))
            f_host, f_dev = self._L.ngd_run_batch, self._L.ngd_run_batch_device
        else:
            a = np.ascontiguousarray(mult, dtype=np.uint32)
            ap = a.ctypes.data_as(C.POINTER(C.c_uint32))
            f_host, f_dev = self._L.ngd_run_mult_batch, self._L.ngd_run_mult_batch_device
        if a.ndim != 2:
            raise ValueError("expected [n_rep][n_blocks]")
        n_rep, n_blocks = a.shape
        if d_sum_ptr is not None:
            _check(f_dev(self._h, ap, n_rep, n_blocks, int(block_size), C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr)))
            return None
        s = np.empty((n_rep, self.n_pairs), dtype=np.float64)
        c = np.empty((n_rep, self.n_pairs), dtype=np.uint64)
        _check(f_host(self._h, ap, n_rep, n_blocks, int(block_size), s.ctypes.data_as(C.POINTER(C.c_double)),
                      c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_job(self, block_maps=None, block_size=1, d_sum_ptr=None, d_cnt_ptr=None):
        """the whole replicate loop in one call (ngd_run_job): matrix 0 = full data, then one matrix per row of
        block_maps ([n_rep][n_blocks]); returns (sum, cnt) of shape [n_rep + 1][n_pairs]"""
        if block_maps is None or len(block_maps) == 0:
            a, ap, n_rep, n_blocks = None, None, 0, 0
        else:
            a = np.ascontiguousarray(block_maps, dtype=np.uint64)
            if a.ndim != 2:
                raise ValueError("expected [n_rep][n_blocks]")
            ap = a.ctypes.data_as(C.POINTER(C.c_uint64))
            n_rep, n_blocks = a.shape
        if d_sum_ptr is not None:
            _check(self._L.ngd_run_job_device(self._h, ap, n_rep, n_blocks, int(block_size), C.c_void_p(d_sum_ptr),
                                              C.c_void_p(d_cnt_ptr)))
            return None
        s = np.empty((n_rep + 1, self.n_pairs), dtype=np.float64)
        c = np.empty((n_rep + 1, self.n_pairs), dtype=np.uint64)
        _check(self._L.ngd_run_job(self._h, ap, n_rep, n_blocks, int(block_size), s.ctypes.data_as(C.POINTER(C.c_double)),
                                   c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_job_dist(self, block_maps=None, block_size=1, evol_model=0, mult=None, out=None, tot_sites=0, lead_full=True):
        """a job and the tail of gen_dist() in one call (ngd_run_job_dist; lead_full=False: ngd_run_batch_dist, mult given:
        ngd_run_mult_batch_dist -- no leading full-data matrix): the finished distances, [n_matrices][n_pairs]; the sums and counts stay in the engine
        (fetch_matrix)"""
        if mult is not None:
            a = np.ascontiguousarray(mult, dtype=np.uint32)
            if a.ndim != 2:
                raise ValueError("expected [n_rep][n_blocks]")
            n_rep, n_blocks = a.shape
            n_mat, fn, ap = n_rep, self._L.ngd_run_mult_batch_dist, a.ctypes.data_as(C.POINTER(C.c_uint32))
        elif block_maps is None or len(block_maps) == 0:
            a, ap, n_rep, n_blocks, n_mat, fn = None, None, 0, 0, 1, self._L.ngd_run_job_dist
        else:
            a = np.ascontiguousarray(block_maps, dtype=np.uint64)
            if a.ndim != 2:
                raise ValueError("expected [n_rep][n_blocks]")
            n_rep, n_blocks = a.shape
            n_mat, fn, ap = n_rep + 1, self._L.ngd_run_job_dist, a.ctypes.data_as(C.POINTER(C.c_uint64))
            if not lead_full:  # replicates only (ngd_run_batch_dist)
                n_mat, fn = n_rep, self._L.ngd_run_batch_dist
        d = np.empty((n_mat, self.n_pairs), dtype=np.float64) if out is None else out
        if d.shape != (n_mat, self.n_pairs) or d.dtype != np.float64 or not d.flags.c_contiguous:
            raise ValueError("out: expected a C-contiguous float64 array [n_matrices][n_pairs]")
        _check(fn(self._h, ap, n_rep, n_blocks, int(block_size), int(tot_sites), int(evol_model), d.ctypes.data_as(C.POINTER(C.c_double))))
        return d

    @staticmethod
    def _win_args(lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        if lo.ndim != 1 or lo.shape != hi.shape:
            raise ValueError("lo, hi: expected two 1-D arrays of the same length")
        return lo, hi, lo.ctypes.data_as(C.POINTER(C.c_uint64)), hi.ctypes.data_as(C.POINTER(C.c_uint64))

    def run_windows(self, lo, hi, d_sum_ptr=None, d_cnt_ptr=None):
        """one matrix per window of sites [lo[w], hi[w]) (ngd_run_windows): -> (sum float64[n_win][n_pairs],
        cnt uint64[n_win][n_pairs]), each what run() gives on the data set cut down to the window; with device pointers
        (ngd_run_windows_device) the results go there and None is returned"""
        lo, hi, lp, hp = self._win_args(lo, hi)
        if d_sum_ptr is not None:
            _check(self._L.ngd_run_windows_device(self._h, lp, hp, lo.size, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr)))
            return None
        s = np.empty((lo.size, self.n_pairs), dtype=np.float64)
        c = np.empty((lo.size, self.n_pairs), dtype=np.uint64)
        _check(self._L.ngd_run_windows(self._h, lp, hp, lo.size, s.ctypes.data_as(C.POINTER(C.c_double)),
                                       c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_windows_dist(self, lo, hi, evol_model=1, tot_sites=0):
        """the windows and the tail of gen_dist() on each (ngd_run_windows_dist): float64[n_win][n_pairs]"""
        lo, hi, lp, hp = self._win_args(lo, hi)
        d = np.empty((lo.size, self.n_pairs), dtype=np.float64)
        _check(self._L.ngd_run_windows_dist(self._h, lp, hp, lo.size, int(tot_sites), int(evol_model),
                                            d.ctypes.data_as(C.POINTER(C.c_double))))
        return d

    @staticmethod
    def _job_maps(block_maps):
        """block maps [n_rep][n_blocks] of a windowed job -> (array kept alive, pointer, n_rep, n_blocks)"""
        if block_maps is None or len(block_maps) == 0:
            return None, None, 0, 0
        a = np.ascontiguousarray(block_maps, dtype=np.uint64)
        if a.ndim != 2:
            raise ValueError("expected [n_rep][n_blocks]")
        return a, a.ctypes.data_as(C.POINTER(C.c_uint64)), a.shape[0], a.shape[1]

    def run_windows_job(self, lo, hi, block_maps, block_size=1, d_sum_ptr=None, d_cnt_ptr=None):
        """bootstrap replicates inside every window (ngd_run_windows_job): windows of ONE length W, block_maps
        [n_rep][W // block_size] shared by all of them; -> (sum, cnt) of shape (n_win, n_rep + 1, n_pairs), matrix 0 of a
        window its full-data matrix, matrix r what run_job() gives for replicate r on the data set cut down to the window;
        with device pointers (ngd_run_windows_job_device) the results go there and None is returned"""
        lo, hi, lp, hp = self._win_args(lo, hi)
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        if d_sum_ptr is not None:
            _check(self._L.ngd_run_windows_job_device(self._h, lp, hp, lo.size, ap, n_rep, n_blocks, int(block_size),
                                                      C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr)))
            return None
        s = np.empty((lo.size, n_rep + 1, self.n_pairs), dtype=np.float64)
        c = np.empty((lo.size, n_rep + 1, self.n_pairs), dtype=np.uint64)
        _check(self._L.ngd_run_windows_job(self._h, lp, hp, lo.size, ap, n_rep, n_blocks, int(block_size),
                                           s.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_windows_job_dist(self, lo, hi, block_maps, block_size=1, evol_model=1, tot_sites=0):
        """the job and the tail of gen_dist() on every matrix (ngd_run_windows_job_dist): float64 (n_win, n_rep + 1, n_pairs)"""
        lo, hi, lp, hp = self._win_args(lo, hi)
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        d = np.empty((lo.size, n_rep + 1, self.n_pairs), dtype=np.float64)
        _check(self._L.ngd_run_windows_job_dist(self._h, lp, hp, lo.size, ap, n_rep, n_blocks, int(block_size), int(tot_sites),
                                                int(evol_model), d.ctypes.data_as(C.POINTER(C.c_double))))
        return d

    @staticmethod
    def _var_maps(block_maps, map_off, n_win):
        """flat block maps and one offset per window (window_boot_maps) -> (arrays kept alive, pointers, entries)"""
        m = np.ascontiguousarray(block_maps if block_maps is not None else [], dtype=np.uint64)
        off = np.ascontiguousarray(map_off, dtype=np.uint64)
        if m.ndim != 1 or off.shape != (n_win,):
            raise ValueError("block_maps: expected a flat array; map_off: one offset per window")
        u64p = C.POINTER(C.c_uint64)
        return (m, off), m.ctypes.data_as(u64p) if m.size else None, off.ctypes.data_as(u64p), m.size

    def run_windows_job_var(self, lo, hi, block_maps, map_off, block_size=1, d_sum_ptr=None, d_cnt_ptr=None, n_rep=None):
        """bootstrap replicates inside windows of UNEQUAL length (ngd_run_windows_job_var): window w draws the maps
        [n_rep][(hi[w] - lo[w]) // block_size] at block_maps[map_off[w]:] (n_rep: read off window_boot_maps()'s layout when
        not given; any other layout must name it); -> (sum, cnt) of shape (n_win, n_rep + 1, n_pairs), a
        window shorter than one block with replicates of sum 0 and count 0; with device pointers
        (ngd_run_windows_job_var_device) the results go there and None is returned"""
        n_win, n_rep, args, keep = self._var_job(lo, hi, block_maps, map_off, block_size, n_rep)
        if d_sum_ptr is not None:
            _check(self._L.ngd_run_windows_job_var_device(*args, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr)))
            return None
        s = np.empty((n_win, n_rep + 1, self.n_pairs), dtype=np.float64)
        c = np.empty((n_win, n_rep + 1, self.n_pairs), dtype=np.uint64)
        _check(self._L.ngd_run_windows_job_var(*args, s.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_windows_job_var_dist(self, lo, hi, block_maps, map_off, block_size=1, evol_model=1, tot_sites=0, n_rep=None):
        """the job and the tail of gen_dist() on every matrix (ngd_run_windows_job_var_dist): float64 (n_win, n_rep + 1,
        n_pairs); the replicates of a window shorter than one block are ngd_finish's 0 / 0"""
        n_win, n_rep, args, keep = self._var_job(lo, hi, block_maps, map_off, block_size, n_rep)
        d = np.empty((n_win, n_rep + 1, self.n_pairs), dtype=np.float64)
        _check(self._L.ngd_run_windows_job_var_dist(*args, int(tot_sites), int(evol_model), d.ctypes.data_as(C.POINTER(C.c_double))))
        return d

    @staticmethod
    def _var_n_rep(lo, hi, off, n_ent, block_size):
        """replicates of a layout window_boot_maps() made: the classes lie one after the other, so the first class's maps
        end where the next offset above its own begins (or where the table ends)"""
        nb = (hi - lo) // np.uint64(max(1, int(block_size)))
        has = np.flatnonzero(nb > 0)
        if has.size == 0:
            raise ValueError("n_rep: no window has a block to tell it from; pass n_rep")
        w = has[np.argmin(off[has])]
        above = off[has][off[has] > off[w]]
        end = int(above.min()) if above.size else int(n_ent)
        return (end - int(off[w])) // int(nb[w])

    def _var_job(self, lo, hi, block_maps, map_off, block_size, n_rep):
        """what every ngd_run_windows_job_var* call starts with -> (n_win, n_rep, the call's leading arguments up to
        block_size, the arrays behind their pointers: to be kept alive until the call is over)"""
        lo, hi, lp, hp = self._win_args(lo, hi)
        keep, mp, op, n_ent = self._var_maps(block_maps, map_off, lo.size)
        n_rep = self._var_n_rep(lo, hi, keep[1], n_ent, block_size) if n_rep is None else int(n_rep)
        return lo.size, n_rep, (self._h, lp, hp, lo.size, mp, n_ent, op, n_rep, int(block_size)), (lo, hi) + keep

    def windows_info(self):
        """what the last windowed call did (ngd_last_windows): segments, slab_bytes, batches, band_launches,
        windows_by_pass, fixup_pairs, ms"""
        t = _lib.NgdWindowsInfo()
        _check(self._L.ngd_last_windows(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    # -- group means: the G x G table of mean distances instead of the n x n matrix -------------------------------
    def set_groups(self, group_of, n_groups=None):
        """the engine's grouping (ngd_set_groups): group_of[i] in [0, n_groups) names individual i's group, -1 leaves it out;
        n_groups: max + 1 when not given; set_groups(None) clears the grouping and frees its device memory"""
        if group_of is None:
            _check(self._L.ngd_set_groups(self._h, None, 0))
            self.n_groups = 0
            return self
        g = np.ascontiguousarray(group_of, dtype=np.int32)
        if g.shape != (self.n_ind,):
            raise ValueError("group_of: expected one entry per individual")
        n_groups = int(g.max()) + 1 if n_groups is None else int(n_groups)
        _check(self._L.ngd_set_groups(self._h, g.ctypes.data_as(C.POINTER(C.c_int32)), n_groups))
        self.n_groups = n_groups
        return self

    def _group_out(self, *lead):
        n_gp = n_group_pairs(getattr(self, "n_groups", 0))
        mean = np.empty(lead + (n_gp,), dtype=np.float64)
        used = np.empty(lead + (n_gp,), dtype=np.uint64)
        return mean, used, mean.ctypes.data_as(C.POINTER(C.c_double)), used.ctypes.data_as(C.POINTER(C.c_uint64))

    def group_means(self, d_sum_ptr, d_cnt_ptr, n_mat, evol_model=1, tot_sites=0):
        """the group reduction of n_mat device matrices (ngd_group_means_device; raw addresses of [n_mat][n_pairs] sums and
        counts, as a *_device call wrote them): -> (mean float64[n_mat][n_gp], used uint64[n_mat][n_gp]), the mean of the
        finite cells of every pair of groups (NaN where there is none) and their number"""
        mean, used, mp, up = self._group_out(int(n_mat))
        _check(self._L.ngd_group_means_device(self._h, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr), int(n_mat), int(tot_sites),
                                              int(evol_model), mp, up))
        return mean, used

    def run_job_groups(self, block_maps=None, block_size=1, evol_model=1, tot_sites=0):
        """run_job() and the group reduction of its matrices on the device (ngd_run_job_groups): -> (mean, used) of shape
        (n_rep + 1, n_gp)"""
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        mean, used, mp, up = self._group_out(n_rep + 1)
        _check(self._L.ngd_run_job_groups(self._h, ap, n_rep, n_blocks, int(block_size), int(tot_sites), int(evol_model), mp, up))
        return mean, used

    def run_windows_groups(self, lo, hi, evol_model=1, tot_sites=0):
        """run_windows() and the group reduction of every window (ngd_run_windows_groups): -> (mean, used) of shape (n_win, n_gp)"""
        lo, hi, lp, hp = self._win_args(lo, hi)
        mean, used, mp, up = self._group_out(lo.size)
        _check(self._L.ngd_run_windows_groups(self._h, lp, hp, lo.size, int(tot_sites), int(evol_model), mp, up))
        return mean, used

    def run_windows_job_var_groups(self, lo, hi, block_maps, map_off, block_size=1, evol_model=1, tot_sites=0, n_rep=None):
        """run_windows_job_var() and the group reduction of every matrix (ngd_run_windows_job_var_groups): -> (mean, used) of
        shape (n_win, n_rep + 1, n_gp)"""
        n_win, n_rep, args, keep = self._var_job(lo, hi, block_maps, map_off, block_size, n_rep)
        mean, used, mp, up = self._group_out(n_win, n_rep + 1)
        _check(self._L.ngd_run_windows_job_var_groups(*args, int(tot_sites), int(evol_model), mp, up))
        return mean, used

    def groups_ms(self):
        """device time of the group reduction's kernels in the last *_groups / group_means call (ngd_last_groups_ms)"""
        v = C.c_double(0.0)
        _check(self._L.ngd_last_groups_ms(self._h, C.byref(v)))
        return float(v.value)

    # -- bootstrap summaries: per cell est, mean, sd, lo, hi over a set's replicates instead of its R + 1 matrices ------
    @staticmethod
    def _stats_out(lead, n_cells):
        stats = np.empty(lead + (_lib.NSTAT, n_cells), dtype=np.float64)
        used = np.empty(lead + (n_cells,), dtype=np.uint64)
        return stats, used, stats.ctypes.data_as(C.POINTER(C.c_double)), used.ctypes.data_as(C.POINTER(C.c_uint64))

    def boot_stats(self, d_sum_ptr, d_cnt_ptr, n_set, n_mat, evol_model=1, tot_sites=0, ci=0.95):
        """the summaries of device matrices (ngd_boot_stats_device; raw addresses of [n_set][n_mat][n_pairs] sums and counts,
        as a *_device call wrote them): -> (stats float64[n_set][5][n_pairs], used uint64[n_set][n_pairs]); stats are est,
        mean, sd, lo, hi of every cell over the finite ones of its n_mat - 1 replicates, used their number"""
        stats, used, sp, up = self._stats_out((int(n_set),), self.n_pairs)
        _check(self._L.ngd_boot_stats_device(self._h, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr), int(n_set), int(n_mat),
                                             int(tot_sites), int(evol_model), float(ci), sp, up))
        return stats, used

    def boot_stats_values(self, d_val_ptr, n_set, n_mat, n_cells, ci=0.95):
        """the summaries of [n_set][n_mat][n_cells] float64 values in device memory as they are
        (ngd_boot_stats_values_device): -> (stats float64[n_set][5][n_cells], used uint64[n_set][n_cells])"""
        stats, used, sp, up = self._stats_out((int(n_set),), int(n_cells))
        _check(self._L.ngd_boot_stats_values_device(self._h, C.c_void_p(d_val_ptr), int(n_set), int(n_mat), int(n_cells),
                                                    float(ci), sp, up))
        return stats, used

    def run_job_stats(self, block_maps, block_size=1, evol_model=1, tot_sites=0, ci=0.95):
        """run_job() and the summaries of its one set on the device (ngd_run_job_stats): -> (stats float64[5][n_pairs],
        used uint64[n_pairs])"""
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        stats, used, sp, up = self._stats_out((), self.n_pairs)
        _check(self._L.ngd_run_job_stats(self._h, ap, n_rep, n_blocks, int(block_size), int(tot_sites), int(evol_model),
                                         float(ci), sp, up))
        return stats, used

    def run_job_groups_stats(self, block_maps, block_size=1, evol_model=1, tot_sites=0, ci=0.95):
        """run_job(), the group reduction of its matrices and the summaries of the means, all on the device
        (ngd_run_job_groups_stats): -> (stats float64[5][n_gp], used uint64[n_gp])"""
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        stats, used, sp, up = self._stats_out((), n_group_pairs(getattr(self, "n_groups", 0)))
        _check(self._L.ngd_run_job_groups_stats(self._h, ap, n_rep, n_blocks, int(block_size), int(tot_sites), int(evol_model),
                                                float(ci), sp, up))
        return stats, used

    def _windows_stats(self, fn, n_cells, lo, hi, block_maps, map_off, block_size, evol_model, tot_sites, n_rep, ci):
        n_win, n_rep, args, keep = self._var_job(lo, hi, block_maps, map_off, block_size, n_rep)
        stats, used, sp, up = self._stats_out((n_win,), n_cells)
        _check(fn(*args, int(tot_sites), int(evol_model), float(ci), sp, up))
        return stats, used

    def run_windows_job_var_stats(self, lo, hi, block_maps, map_off, block_size=1, evol_model=1, tot_sites=0, n_rep=None, ci=0.95):
        """run_windows_job_var() and the summaries of every window's set (ngd_run_windows_job_var_stats): -> (stats
        float64[n_win][5][n_pairs], used uint64[n_win][n_pairs]); a window shorter than one block has used = 0"""
        return self._windows_stats(self._L.ngd_run_windows_job_var_stats, self.n_pairs, lo, hi, block_maps, map_off, block_size,
                                   evol_model, tot_sites, n_rep, ci)

    def run_windows_job_var_groups_stats(self, lo, hi, block_maps, map_off, block_size=1, evol_model=1, tot_sites=0, n_rep=None,
                                         ci=0.95):
        """run_windows_job_var(), the group reduction and the summaries of every window's means
        (ngd_run_windows_job_var_groups_stats): -> (stats float64[n_win][5][n_gp], used uint64[n_win][n_gp])"""
        return self._windows_stats(self._L.ngd_run_windows_job_var_groups_stats, n_group_pairs(getattr(self, "n_groups", 0)), lo, hi,
                                   block_maps, map_off, block_size, evol_model, tot_sites, n_rep, ci)

    def last_boot_stats_ms(self):
        """device time of the summary kernels in the last of these calls (ngd_last_boot_stats_ms)"""
        v = C.c_double(0.0)
        _check(self._L.ngd_last_boot_stats_ms(self._h, C.byref(v)))
        return float(v.value)

    # -- neighbour-joining trees: per matrix 2 n - 3 branches (child, len) and a status instead of its n_pairs cells ----
    def _nj_out(self, lead, dist0_lead=None):
        nb = 2 * self.n_ind - 3
        child = np.empty(lead + (nb,), dtype=np.int32)
        length = np.empty(lead + (nb,), dtype=np.float64)
        status = np.empty(lead, dtype=np.uint32)
        dist0 = None if dist0_lead is None else np.empty(dist0_lead + (self.n_pairs,), dtype=np.float64)
        return (child, length, status, dist0, child.ctypes.data_as(C.POINTER(C.c_int32)), length.ctypes.data_as(C.POINTER(C.c_double)),
                status.ctypes.data_as(C.POINTER(C.c_uint32)), None if dist0 is None else dist0.ctypes.data_as(C.POINTER(C.c_double)))

    def nj(self, d_sum_ptr, d_cnt_ptr, n_mat, evol_model=1, tot_sites=0):
        """the neighbour-joining trees of device matrices (ngd_nj_device; raw addresses of [n_mat][n_pairs] sums and counts,
        as a *_device call wrote them): -> (child int32[n_mat][2n-3], len float64[n_mat][2n-3], status uint32[n_mat]);
        join t makes node n + t of entries 2t, 2t + 1, the last three entries meet at the centre; status 0 (child -1, len
        NaN): a matrix with a cell that is not finite"""
        child, length, status, _, cp, lp, sp, _ = self._nj_out((int(n_mat),))
        _check(self._L.ngd_nj_device(self._h, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr), int(n_mat), int(tot_sites),
                                     int(evol_model), cp, lp, sp))
        return child, length, status

    def nj_values(self, d_val_ptr, n_mat):
        """the trees of [n_mat][n_pairs] float64 distances in device memory as they are (ngd_nj_values_device)"""
        child, length, status, _, cp, lp, sp, _ = self._nj_out((int(n_mat),))
        _check(self._L.ngd_nj_values_device(self._h, C.c_void_p(d_val_ptr), int(n_mat), cp, lp, sp))
        return child, length, status

    def run_job_nj(self, block_maps=None, block_size=1, evol_model=1, tot_sites=0, dist0=True):
        """run_job() and the trees of its n_rep + 1 matrices on the device (ngd_run_job_nj): -> (child, len, status, dist0)
        of shapes (n_rep + 1, 2n-3), (n_rep + 1, 2n-3), (n_rep + 1,), (n_pairs,); dist0 (None with dist0=False) is matrix 0
        as run_job_dist() gives it"""
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        child, length, status, d0, cp, lp, sp, dp = self._nj_out((n_rep + 1,), () if dist0 else None)
        _check(self._L.ngd_run_job_nj(self._h, ap, n_rep, n_blocks, int(block_size), int(tot_sites), int(evol_model), cp, lp, sp, dp))
        return child, length, status, d0

    def run_windows_nj(self, lo, hi, evol_model=1, tot_sites=0, dist0=True):
        """run_windows() and every window's tree (ngd_run_windows_nj): -> (child (n_win, 1, 2n-3), len, status (n_win, 1),
        dist0 (n_win, n_pairs))"""
        lo, hi, lp_, hp = self._win_args(lo, hi)
        child, length, status, d0, cp, lp, sp, dp = self._nj_out((lo.size, 1), (lo.size,) if dist0 else None)
        _check(self._L.ngd_run_windows_nj(self._h, lp_, hp, lo.size, int(tot_sites), int(evol_model), cp, lp, sp, dp))
        return child, length, status, d0

    def run_windows_job_var_nj(self, lo, hi, block_maps, map_off, block_size=1, evol_model=1, tot_sites=0, n_rep=None, dist0=True):
        """run_windows_job_var() and the trees of every window's set (ngd_run_windows_job_var_nj): -> (child (n_win,
        n_rep + 1, 2n-3), len, status (n_win, n_rep + 1), dist0 (n_win, n_pairs)); the replicates of a window shorter than
        one block have status 0"""
        n_win, n_rep, args, keep = self._var_job(lo, hi, block_maps, map_off, block_size, n_rep)
        child, length, status, d0, cp, lp, sp, dp = self._nj_out((n_win, n_rep + 1), (n_win,) if dist0 else None)
        _check(self._L.ngd_run_windows_job_var_nj(*args, int(tot_sites), int(evol_model), cp, lp, sp, dp))
        return child, length, status, d0

    def last_nj_ms(self):
        """device time of the tree kernels in the last of these calls (ngd_last_nj_ms)"""
        v = C.c_double(0.0)
        _check(self._L.ngd_last_nj_ms(self._h, C.byref(v)))
        return float(v.value)

    # -- classical MDS: per matrix its top K eigenpairs, the two sums of its eigenvalues and a status ----
    def _mds_out(self, lead, K, dist0_lead=None):
        K = int(K)
        eig = np.empty(lead + (K,), dtype=np.float64)
        vec = np.empty(lead + (K, self.n_ind), dtype=np.float64)
        tot = np.empty(lead + (2,), dtype=np.float64)
        status = np.empty(lead, dtype=np.uint32)
        dist0 = None if dist0_lead is None else np.empty(dist0_lead + (self.n_pairs,), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        return ((eig, vec, tot, status, dist0),
                (K, eig.ctypes.data_as(dp), vec.ctypes.data_as(dp), tot.ctypes.data_as(dp), status.ctypes.data_as(C.POINTER(C.c_uint32))),
                None if dist0 is None else dist0.ctypes.data_as(dp))

    def mds(self, d_sum_ptr, d_cnt_ptr, n_mat, K, evol_model=1, tot_sites=0):
        """classical MDS of device matrices (ngd_mds_device; raw addresses of [n_mat][n_pairs] sums and counts, as a
        *_device call wrote them): -> (eig float64[n_mat][K], the largest eigenvalues of the double-centred matrix in
        descending order; vec float64[n_mat][K][n], their unit vectors; tot float64[n_mat][2], the sum of all eigenvalues
        and of the positive ones; status uint32[n_mat]); status 0 (everything NaN): a matrix with a cell that is not finite"""
        out, args, _ = self._mds_out((int(n_mat),), K)
        _check(self._L.ngd_mds_device(self._h, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr), int(n_mat), int(tot_sites),
                                      int(evol_model), *args))
        return out[:4]

    def mds_values(self, d_val_ptr, n_mat, K):
        """the same of [n_mat][n_pairs] float64 distances in device memory as they are (ngd_mds_values_device)"""
        out, args, _ = self._mds_out((int(n_mat),), K)
        _check(self._L.ngd_mds_values_device(self._h, C.c_void_p(d_val_ptr), int(n_mat), *args))
        return out[:4]

    def run_job_mds(self, K, block_maps=None, block_size=1, evol_model=1, tot_sites=0, dist0=True):
        """run_job() and the MDS of its n_rep + 1 matrices on the device (ngd_run_job_mds): -> (eig (n_rep + 1, K), vec
        (n_rep + 1, K, n), tot (n_rep + 1, 2), status (n_rep + 1,), dist0 (n_pairs,)); dist0 (None with dist0=False) is
        matrix 0 as run_job_dist() gives it"""
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        out, args, dp = self._mds_out((n_rep + 1,), K, () if dist0 else None)
        _check(self._L.ngd_run_job_mds(self._h, ap, n_rep, n_blocks, int(block_size), int(tot_sites), int(evol_model), *args, dp))
        return out

    def run_windows_mds(self, K, lo, hi, evol_model=1, tot_sites=0, dist0=True):
        """run_windows() and every window's MDS (ngd_run_windows_mds): -> (eig (n_win, 1, K), vec (n_win, 1, K, n), tot
        (n_win, 1, 2), status (n_win, 1), dist0 (n_win, n_pairs))"""
        lo, hi, lp_, hp = self._win_args(lo, hi)
        out, args, dp = self._mds_out((lo.size, 1), K, (lo.size,) if dist0 else None)
        _check(self._L.ngd_run_windows_mds(self._h, lp_, hp, lo.size, int(tot_sites), int(evol_model), *args, dp))
        return out

    def run_windows_job_var_mds(self, K, lo, hi, block_maps, map_off, block_size=1, evol_model=1, tot_sites=0, n_rep=None, dist0=True):
        """run_windows_job_var() and the MDS of every window's set (ngd_run_windows_job_var_mds): -> (eig (n_win, n_rep + 1,
        K), vec, tot, status (n_win, n_rep + 1), dist0 (n_win, n_pairs)); the replicates of a window shorter than one block
        have status 0"""
        n_win, n_rep, wargs, keep = self._var_job(lo, hi, block_maps, map_off, block_size, n_rep)
        out, args, dp = self._mds_out((n_win, n_rep + 1), K, (n_win,) if dist0 else None)
        _check(self._L.ngd_run_windows_job_var_mds(*wargs, int(tot_sites), int(evol_model), *args, dp))
        return out

    def last_mds_ms(self):
        """device time of the MDS kernels in the last of these calls (ngd_last_mds_ms)"""
        v = C.c_double(0.0)
        _check(self._L.ngd_last_mds_ms(self._h, C.byref(v)))
        return float(v.value)

    # -- comparison of windows: per vector its mean and status, per pair of vectors the centred Gram entry ----
    @staticmethod
    def _win_cmp_out(W):
        mean = np.empty(W, dtype=np.float64)
        gram = np.empty((W, W), dtype=np.float64)
        status = np.empty(W, dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        return (mean, gram, status), (mean.ctypes.data_as(dp), gram.ctypes.data_as(dp), status.ctypes.data_as(C.POINTER(C.c_uint32)))

    def win_cmp(self, d_sum_ptr, d_cnt_ptr, n_vec, evol_model=1, tot_sites=0):
        """the windows of device matrices compared (ngd_win_cmp_device; raw addresses of [n_vec][n_pairs] sums and counts, as
        run_windows_device() wrote them): -> (mean float64[n_vec], gram float64[n_vec][n_vec], status uint32[n_vec]); status
        0 (mean, row and column NaN): a matrix with a cell that is not finite.  win_cmp_finish() derives cor and rms"""
        out, args = self._win_cmp_out(int(n_vec))
        _check(self._L.ngd_win_cmp_device(self._h, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr), int(n_vec), int(tot_sites),
                                          int(evol_model), *args))
        return out

    def win_cmp_values(self, d_val_ptr, n_vec, n_cells):
        """the same of [n_vec][n_cells] float64 vectors in device memory as they are (ngd_win_cmp_values_device); n_cells is
        free of the engine's n_ind"""
        out, args = self._win_cmp_out(int(n_vec))
        _check(self._L.ngd_win_cmp_values_device(self._h, C.c_void_p(d_val_ptr), int(n_vec), int(n_cells), *args))
        return out

    def run_windows_cmp(self, lo, hi, evol_model=1, tot_sites=0, dist=True):
        """run_windows() and the comparison of its windows on the device (ngd_run_windows_cmp): -> (mean (n_win,), gram
        (n_win, n_win), status (n_win,), dist (n_win, n_pairs)); dist (None with dist=False) is run_windows_dist()'s"""
        lo, hi, lp_, hp = self._win_args(lo, hi)
        out, args = self._win_cmp_out(lo.size)
        d = np.empty((lo.size, self.n_pairs), dtype=np.float64) if dist else None
        _check(self._L.ngd_run_windows_cmp(self._h, lp_, hp, lo.size, int(tot_sites), int(evol_model), *args,
                                           None if d is None else d.ctypes.data_as(C.POINTER(C.c_double))))
        return out + (d,)

    def last_win_cmp_ms(self):
        """device time of the four kernels in the last of these calls (ngd_last_win_cmp_ms): dict of stats, pack, gram, sum"""
        v = (C.c_double * 4)()
        _check(self._L.ngd_last_win_cmp_ms(self._h, v))
        return dict(zip(("stats", "pack", "gram", "sum"), (float(x) for x in v)))

    # -- the MDS replicates of a set rotated onto its matrix 0, and the summaries of the aligned cells ----
    def mds_align_values(self, d_coords_ptr, n_set, n_mat, K, status=None):
        """the alignment alone, of [n_set][n_mat][K][n] float64 coordinates in device memory as they are
        (ngd_mds_align_values_device; status uint32[n_set][n_mat] on the host, None: every matrix has status 1): ->
        (aligned float64[n_set][n_mat][K][n], fit float64[n_set][n_mat]); matrix 0 of a set stays as it is (fit 0), a matrix
        left out is NaN"""
        n_set, n_mat, K = int(n_set), int(n_mat), int(K)
        aligned = np.empty((n_set, n_mat, max(K, 0), self.n_ind), dtype=np.float64)
        fit = np.empty((n_set, n_mat), dtype=np.float64)
        sp = None
        if status is not None:
            st = np.ascontiguousarray(status, dtype=np.uint32)
            if st.size != n_set * n_mat:
                raise ValueError("status: expected [n_set][n_mat]")
            sp = st.ctypes.data_as(C.POINTER(C.c_uint32))
        dp = C.POINTER(C.c_double)
        _check(self._L.ngd_mds_align_values_device(self._h, C.c_void_p(d_coords_ptr), sp, n_set, n_mat, K, aligned.ctypes.data_as(dp),
                                                   fit.ctypes.data_as(dp)))
        return aligned, fit

    def _mds_align_out(self, lead, n_mat, K, aligned, dist0):
        K, n = int(K), self.n_ind
        nc = max(K, 0) * (n + 1)
        out = {"eig0": np.empty(lead + (max(K, 0),)), "vec0": np.empty(lead + (max(K, 0), n)), "tot0": np.empty(lead + (2,)),
               "status": np.empty(lead + (n_mat,), dtype=np.uint32), "stats": np.empty(lead + (_lib.NSTAT, nc)),
               "used": np.empty(lead, dtype=np.uint64), "fit": np.empty(lead + (n_mat,)),
               "aligned": np.empty(lead + (n_mat, max(K, 0), n)) if aligned else None,
               "dist0": np.empty(lead + (self.n_pairs,)) if dist0 else None}
        ptr = {np.dtype(np.float64): C.POINTER(C.c_double), np.dtype(np.uint32): C.POINTER(C.c_uint32),
               np.dtype(np.uint64): C.POINTER(C.c_uint64)}
        args = [None if v is None else v.ctypes.data_as(ptr[v.dtype]) for v in out.values()]
        return out, args

    def run_job_mds_align(self, K, block_maps, block_size=1, evol_model=1, tot_sites=0, ci=0.95, aligned=True, dist0=True):
        """run_job_mds(), the replicates rotated onto matrix 0 and the summaries of the aligned cells, all on the device
        (ngd_run_job_mds_align): -> dict of eig0 (K,), vec0 (K, n), tot0 (2,) -- matrix 0's, as run_job_mds() gives them --,
        status (n_rep + 1,), stats (5, K (n + 1)) -- est, mean, sd, lo, hi of the cells [K][n], then of the K eigenvalues --,
        used (the replicates that went in), fit (n_rep + 1,), aligned (n_rep + 1, K, n) or None, dist0 (n_pairs,) or None"""
        a, ap, n_rep, n_blocks = self._job_maps(block_maps)
        out, args = self._mds_align_out((), n_rep + 1, K, aligned, dist0)
        _check(self._L.ngd_run_job_mds_align(self._h, ap, n_rep, n_blocks, int(block_size), int(tot_sites), int(evol_model), int(K),
                                             float(ci), *args))
        return out

    def run_windows_job_var_mds_align(self, K, lo, hi, block_maps, map_off, block_size=1, evol_model=1, tot_sites=0, n_rep=None,
                                      ci=0.95, aligned=True, dist0=True):
        """the same for every window's set (ngd_run_windows_job_var_mds_align): the dict's arrays with a leading n_win; the
        replicates of a window shorter than one block are left out (used 0, the statistics but est NaN)"""
        n_win, n_rep, wargs, keep = self._var_job(lo, hi, block_maps, map_off, block_size, n_rep)
        out, args = self._mds_align_out((n_win,), n_rep + 1, K, aligned, dist0)
        _check(self._L.ngd_run_windows_job_var_mds_align(*wargs, int(tot_sites), int(evol_model), int(K), float(ci), *args))
        return out

    def last_mds_align_ms(self):
        """device time of the two alignment kernels in the last of these calls (ngd_last_mds_align_ms)"""
        v = C.c_double(0.0)
        _check(self._L.ngd_last_mds_align_ms(self._h, C.byref(v)))
        return float(v.value)

    def run_job_keep(self, block_maps, block_size=1):
        """ngd_run_job with the matrices left in the engine; fetch_matrix(r) copies them out one at a time"""
        a = np.ascontiguousarray(block_maps, dtype=np.uint64)
        n_rep, n_blocks = a.shape
        _check(self._L.ngd_run_job(self._h, a.ctypes.data_as(C.POINTER(C.c_uint64)), n_rep, n_blocks, int(block_size), None, None))
        return n_rep + 1

    def fetch_matrix(self, which):
        s = np.empty(self.n_pairs, dtype=np.float64)
        c = np.empty(self.n_pairs, dtype=np.uint64)
        _check(self._L.ngd_fetch_matrix(self._h, int(which), s.ctypes.data_as(C.POINTER(C.c_double)),
                                        c.ctypes.data_as(C.POINTER(C.c_uint64))))
        return s, c

    def run_device(self, d_sum_ptr, d_cnt_ptr, block_map=None, block_size=1):
        """Results written to caller-owned device buffers (raw addresses)."""
        ptr, nb, bs, keep = self._map_args(block_map, block_size)
        _check(self._L.ngd_run_device(self._h, ptr, nb, bs, C.c_void_p(d_sum_ptr), C.c_void_p(d_cnt_ptr)))

    def set_option(self, name, value):
        """plan selection for the replicate loop (ngd_set_option): boot_partials, boot_max_bytes, boot_wg, boot_unaligned,
        em_batch, em_spill, em_spill_bytes, single_image_bytes, fixup_work, win_plan, win_max_bytes; em_exact (the plain
        pass of the table-driven EM kernel stops where the reference does: last_em_exact(), em_exact_entries(); 2: block
        maps, multiplicities, batches and jobs are served that way too) and em_exact_cap; em_exact_win (1: while em_exact is on the windowed calls
        are served too -- run_windows* under 1 or 2, run_windows_job* under 2); unit_skip (0: the plain pass of a
        one-image engine in congruent coordinates visits the k-groups of p0 + p1 + p2 too: plain_pass_kgroups());
        nj_max_bytes (device scratch of the neighbour-joining kernel, 0 = 2 GB: the matrices a launch takes);
        mds_max_bytes (the same for the classical-MDS kernel); win_cmp_max_bytes (device memory of the comparison of windows,
        0 = half of what is free at the call: a call that needs more is refused)"""
        _check(self._L.ngd_set_option(self._h, OPTIONS[name], int(value)))
        return self

    def drop_caches(self):
        """forget the bootstrap block partial sums (benchmarks: charge them to every step)"""
        _check(self._L.ngd_drop_caches(self._h))

    def timing(self):
        t = _lib.NgdTiming()
        _check(self._L.ngd_last_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def plain_pass_kgroups(self):
        """k-groups the last plain pass of an MFMA engine visited (ngd_last_plain_pass): two thirds of the image's where the
        unit_skip option applied"""
        n = C.c_uint64(0)
        _check(self._L.ngd_last_plain_pass(self._h, C.byref(n)))
        return int(n.value)

    def spill_timing(self):
        """the spilled-terms plan's accumulation phase kernel by kernel (ngd_last_spill_timing); zeros after another plan"""
        t = _lib.NgdSpillTiming()
        _check(self._L.ngd_last_spill_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def image_mode(self):
        """(what the engine holds: 3 two images / 1 / 2, 0 = not an MFMA engine; whether it recomputes nearly identical pairs)"""
        f = C.c_int(0)
        m = self._L.ngd_image_mode(self._h, C.byref(f))
        return int(m), bool(f.value)

    def fixup(self):
        """the fix-up pass of the last run (ngd_last_fixup): flagged / recomputed / skipped pairs, ms"""
        t = _lib.NgdFixupInfo()
        _check(self._L.ngd_last_fixup(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def last_em_exact(self):
        """the recheck of the last plain pass under the em_exact option (ngd_last_em_exact): noted, changed, passes, ms"""
        t = _lib.NgdEmExactInfo()
        _check(self._L.ngd_last_em_exact(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def em_exact_entries(self):
        """the noted (pair, site)s of that pass, sorted by (i1, i2, site) (ngd_em_exact_entries): a structured array with
        i1, i2, site, t_dev, t_ref, c_dev, c_ref"""
        n = self._L.ngd_em_exact_entries(self._h, None, 0)
        if n < 0:
            _check(int(n))
        out = np.zeros(int(n), dtype=EM_EXACT_ENTRY)
        if n:
            self._L.ngd_em_exact_entries(self._h, out.ctypes.data_as(C.POINTER(_lib.NgdEmExactEntry)), int(n))
        return out

    def em_work(self):
        """table-driven EM kernel: ((tile, site) visits, table rounds) of the last run"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.ngd_last_em_work(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def shader_clock_mhz(self):
        """shader clock of the last MFMA / table-driven EM launch, sampled inside the kernel (0.0: not sampled)"""
        v = C.c_double(0.0)
        _check(self._L.ngd_last_shader_clock(self._h, C.byref(v)))
        return float(v.value)

    def device_bytes(self):
        return int(self._L.ngd_device_bytes(self._h))


def finish(sum_, cnt, tot_sites=0, evol_model=1, out=None):
    """Tail of gen_dist(), ngsDist.cpp:372-401, on the host's libm.  `out` (float64, same size) avoids a fresh
    allocation per call."""
    L = _lib.load()
    s = np.ascontiguousarray(sum_, dtype=np.float64)
    c = np.ascontiguousarray(cnt, dtype=np.uint64)
    if out is None:
        out = np.empty_like(s)
    elif out.dtype != np.float64 or out.size != s.size or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float64 array of the same size")
    _check(L.ngd_finish(s.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_uint64)),
                        s.size, int(tot_sites), int(evol_model), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def em2_site(g1, g2):
    """one site of the reference's two-individual EM (ngd_em2_site: em2() of emOptim2.cpp over a 3 x 3 sfs that starts at
    1/9, tolerance 0.001, at most 50 steps) on the host: -> (sfs float64[9], number of EM steps).  Needs no device."""
    L = _lib.load()
    a = np.ascontiguousarray(g1, dtype=np.float64).reshape(3)
    b = np.ascontiguousarray(g2, dtype=np.float64).reshape(3)
    sfs = np.full(9, 1.0 / 9)
    n = C.c_int(0)
    dp = C.POINTER(C.c_double)
    L.ngd_em2_site(a.ctypes.data_as(dp), b.ctypes.data_as(dp), sfs.ctypes.data_as(dp), C.byref(n))
    return sfs, int(n.value)


def window_ranges(n_sites, size, step=None, chrom=None):
    """the window list of --win_size / --win_step (ngd_window_ranges): -> (lo, hi) uint64 arrays.  chrom: one id per site
    (any hashable values; a chromosome is a maximal run of equal ids and must not come back after another one)."""
    L = _lib.load()
    step = size if step is None else step
    ids = None
    if chrom is not None:
        if len(chrom) != n_sites:
            raise ValueError("chrom: expected one id per site")
        codes = {}
        ids = np.fromiter((codes.setdefault(c, len(codes)) for c in chrom), dtype=np.uint32, count=n_sites)
    idp = ids.ctypes.data_as(C.POINTER(C.c_uint32)) if ids is not None else None
    n = L.ngd_window_ranges(idp, int(n_sites), int(size), int(step), None, None, 0)
    if n < 0:
        raise NgdError(int(n), "window_ranges: size and step must be positive and chromosomes grouped")
    lo = np.zeros(n, dtype=np.uint64)
    hi = np.zeros(n, dtype=np.uint64)
    L.ngd_window_ranges(idp, int(n_sites), int(size), int(step), lo.ctypes.data_as(C.POINTER(C.c_uint64)),
                        hi.ctypes.data_as(C.POINTER(C.c_uint64)), n)
    return lo, hi


def window_ranges_bp(pos, size, step=None, chrom=None, min_sites=1):
    """the window list of --win_bp / --win_bp_step (ngd_window_ranges_bp): -> (lo, hi, bp_start) uint64 arrays.  pos: one
    coordinate >= 1 per site, not descending inside a chromosome; window k of a chromosome covers the coordinates
    [1 + k step, 1 + k step + size), its sites are [lo, hi), and windows with fewer than max(1, min_sites) sites are left
    out.  chrom: as window_ranges()."""
    L = _lib.load()
    step = size if step is None else step
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    if pos.ndim != 1:
        raise ValueError("pos: expected one coordinate per site")
    n_sites = pos.size
    ids = None
    if chrom is not None:
        if len(chrom) != n_sites:
            raise ValueError("chrom: expected one id per site")
        codes = {}
        ids = np.fromiter((codes.setdefault(c, len(codes)) for c in chrom), dtype=np.uint32, count=n_sites)
    u64p = C.POINTER(C.c_uint64)
    idp = ids.ctypes.data_as(C.POINTER(C.c_uint32)) if ids is not None else None
    args = (idp, pos.ctypes.data_as(u64p), n_sites, int(size), int(step), int(min_sites))
    n = L.ngd_window_ranges_bp(*args, None, None, None, 0)
    if n < 0:
        raise NgdError(int(n), "window_ranges_bp: size and step must be positive, positions whole numbers from 1 to 2^62 that "
                               "do not descend inside a chromosome, and chromosomes grouped")
    lo, hi, start = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    L.ngd_window_ranges_bp(*args, lo.ctypes.data_as(u64p), hi.ctypes.data_as(u64p), start.ctypes.data_as(u64p), n)
    return lo, hi, start


def window_boot_maps(seed, lo, hi, n_rep, block_size):
    """the block maps of run_windows_job_var() (ngd_window_boot_maps), drawn as the reference would on every window's
    cut-down file: -> (block_maps uint64[entries], map_off uint64[n_win]); window w's maps are
    block_maps[map_off[w]:][:n_rep * n_blocks_w].reshape(n_rep, n_blocks_w), n_blocks_w = (hi[w] - lo[w]) // block_size"""
    L = _lib.load()
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hi = np.ascontiguousarray(hi, dtype=np.uint64)
    if lo.ndim != 1 or lo.shape != hi.shape:
        raise ValueError("lo, hi: expected two 1-D arrays of the same length")
    u64p = C.POINTER(C.c_uint64)
    off = np.zeros(lo.size, dtype=np.uint64)
    args = (int(seed), lo.ctypes.data_as(u64p), hi.ctypes.data_as(u64p), lo.size, int(n_rep), int(block_size))
    n = L.ngd_window_boot_maps(*args, None, 0, off.ctypes.data_as(u64p))
    if n < 0:
        raise NgdError(int(n), "window_boot_maps: block_size must be positive and no window end before its start")
    maps = np.zeros(n, dtype=np.uint64)
    L.ngd_window_boot_maps(*args, maps.ctypes.data_as(u64p), n, off.ctypes.data_as(u64p))
    return maps, off


def n_group_pairs(n_groups):
    """pairs of groups (a, b), a <= b (ngd_n_group_pairs): G (G + 1) / 2"""
    return int(_lib.load().ngd_n_group_pairs(int(n_groups)))


def group_pair_index(n_groups, a, b):
    """the place of group pair (a, b), a <= b, in the row-major upper triangle with the diagonal (ngd_group_pair_index)"""
    if not 0 <= a <= b < n_groups:
        raise ValueError("expected 0 <= a <= b < n_groups")
    return int(_lib.load().ngd_group_pair_index(int(n_groups), int(a), int(b)))


def group_cells(group_of, n_groups=None):
    """the cells -- pairs of individuals -- of every group pair (ngd_group_cells): uint64[n_gp]; needs no device"""
    g = np.ascontiguousarray(group_of, dtype=np.int32)
    if g.ndim != 1:
        raise ValueError("group_of: expected one entry per individual")
    n_groups = int(g.max()) + 1 if n_groups is None else int(n_groups)
    cells = np.zeros(n_group_pairs(n_groups), dtype=np.uint64)
    rc = _lib.load().ngd_group_cells(g.ctypes.data_as(C.POINTER(C.c_int32)), g.size, n_groups,
                                     cells.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        raise NgdError(int(rc), "group_cells: n_groups must be positive and every entry in [-1, n_groups)")
    return cells


def expand_groups(mean, n_groups):
    """[..., n_gp] in group-pair order -> the symmetric [..., G, G] table (the within-group value on the diagonal)"""
    m = np.asarray(mean)
    if m.shape[-1] != n_group_pairs(n_groups):
        raise ValueError("the last axis must hold n_groups * (n_groups + 1) / 2 entries")
    a, b = np.triu_indices(n_groups)
    out = np.empty(m.shape[:-1] + (n_groups, n_groups), dtype=m.dtype)
    out[..., a, b] = m
    out[..., b, a] = m
    return out


def boot_stats_max_rep():
    """the most replicates the device's summaries serve (ngd_boot_stats_max_rep): a cell's values stay in on-chip memory"""
    return int(_lib.load().ngd_boot_stats_max_rep())


def boot_stats_host(values, ci=0.95):
    """the summaries in plain host arithmetic (ngd_boot_stats_host), for callers of the *_dist forms: values
    float64[..., n_mat, n_cells], matrix 0 the estimate and the others its replicates -> (stats float64[..., 5, n_cells] =
    est, mean, sd, lo, hi; used uint64[..., n_cells])"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.ndim < 2:
        raise ValueError("values: expected [..., n_mat, n_cells]")
    lead, (n_mat, n_cells) = v.shape[:-2], v.shape[-2:]
    n_set = int(np.prod(lead, dtype=np.int64))
    stats = np.empty(lead + (_lib.NSTAT, n_cells), dtype=np.float64)
    used = np.empty(lead + (n_cells,), dtype=np.uint64)
    _check(_lib.load().ngd_boot_stats_host(v.ctypes.data_as(C.POINTER(C.c_double)), n_set, n_mat, n_cells, float(ci),
                                           stats.ctypes.data_as(C.POINTER(C.c_double)), used.ctypes.data_as(C.POINTER(C.c_uint64))))
    return stats, used


def nj_max_ind():
    """the most individuals the device's neighbour joining serves (ngd_nj_max_ind)"""
    return int(_lib.load().ngd_nj_max_ind())


def nj_host(values, n_ind):
    """neighbour joining in plain host arithmetic (ngd_nj_host), the device form's twin: values float64[..., n_pairs] ->
    (child int32[..., 2n-3], len float64[..., 2n-3], status uint32[...])"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    n_ind = int(n_ind)
    if v.ndim < 1 or v.shape[-1] != n_ind * (n_ind - 1) // 2:
        raise ValueError("values: expected [..., n_pairs]")
    lead = v.shape[:-1]
    n_mat = int(np.prod(lead, dtype=np.int64))
    nb = max(0, 2 * n_ind - 3)
    child = np.empty(lead + (nb,), dtype=np.int32)
    length = np.empty(lead + (nb,), dtype=np.float64)
    status = np.empty(lead, dtype=np.uint32)
    _check(_lib.load().ngd_nj_host(v.ctypes.data_as(C.POINTER(C.c_double)), n_mat, n_ind, child.ctypes.data_as(C.POINTER(C.c_int32)),
                                   length.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_uint32))))
    return child, length, status


def nj_support(child, status, n_ind):
    """bootstrap support of matrix 0's tree (ngd_nj_support): child int32[n_mat][2n-3], status uint32[n_mat] -> (support
    uint32[n-3], one per join of matrix 0: the matrices r >= 1 with a tree that has the join's bipartition; n_used, the
    matrices r >= 1 with a tree)"""
    n_ind = int(n_ind)
    c = np.ascontiguousarray(child, dtype=np.int32)
    s = np.ascontiguousarray(status, dtype=np.uint32)
    if c.ndim != 2 or c.shape != (s.size, 2 * n_ind - 3) or s.ndim != 1:
        raise ValueError("child: expected [n_mat][2 n_ind - 3], status [n_mat]")
    sup = np.zeros(max(0, n_ind - 3), dtype=np.uint32)
    used = C.c_uint32(0)
    keep = sup if sup.size else np.zeros(1, dtype=np.uint32)
    _check(_lib.load().ngd_nj_support(c.ctypes.data_as(C.POINTER(C.c_int32)), s.ctypes.data_as(C.POINTER(C.c_uint32)), s.size, n_ind,
                                      keep.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(used)))
    return sup, int(used.value)


def nj_newick(child, length, labels, support=None):
    """one record as a Newick line (ngd_nj_newick): "(x,y,z);\\n", leaves "label:%.10f", internal nodes "(x,y)" + their
    support number (support uint32[n-3], by join) + ":%.10f"; ";\\n" for a record without a tree.  Returns bytes."""
    n_ind = len(labels)
    c = np.ascontiguousarray(child, dtype=np.int32)
    ln = np.ascontiguousarray(length, dtype=np.float64)
    if c.shape != (2 * n_ind - 3,) or ln.shape != c.shape:
        raise ValueError("child, length: expected [2 n_ind - 3]")
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in labels]
    arr = (C.c_char_p * n_ind)(*raw)
    sp = None
    if support is not None:
        sup = np.ascontiguousarray(support, dtype=np.uint32)
        if sup.shape != (n_ind - 3,):
            raise ValueError("support: expected [n_ind - 3]")
        keep = sup if sup.size else np.zeros(1, dtype=np.uint32)
        sp = keep.ctypes.data_as(C.POINTER(C.c_uint32))
    L = _lib.load()
    args = (c.ctypes.data_as(C.POINTER(C.c_int32)), ln.ctypes.data_as(C.POINTER(C.c_double)), n_ind, arr, sp)
    need = L.ngd_nj_newick(*args, None, 0)
    if need < 0:
        _check(int(need))
    buf = C.create_string_buffer(int(need) + 1)
    _check(min(0, int(L.ngd_nj_newick(*args, buf, int(need)))))
    return buf.raw[:int(need)]


def mds_max_ind():
    """the most individuals the device's classical MDS serves (ngd_mds_max_ind)"""
    return int(_lib.load().ngd_mds_max_ind())


def mds_max_dim():
    """the most dimensions K of classical MDS, device and host (ngd_mds_max_dim)"""
    return int(_lib.load().ngd_mds_max_dim())


def mds_host(values, n_ind, K):
    """classical MDS in plain host arithmetic (ngd_mds_host), the device form's twin: values float64[..., n_pairs] ->
    (eig float64[..., K], vec float64[..., K, n], tot float64[..., 2], status uint32[...])"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    n_ind, K = int(n_ind), int(K)
    if v.ndim < 1 or v.shape[-1] != n_ind * (n_ind - 1) // 2:
        raise ValueError("values: expected [..., n_pairs]")
    lead = v.shape[:-1]
    n_mat = int(np.prod(lead, dtype=np.int64))
    Kc = max(K, 0)
    eig = np.empty(lead + (Kc,), dtype=np.float64)
    vec = np.empty(lead + (Kc, n_ind), dtype=np.float64)
    tot = np.empty(lead + (2,), dtype=np.float64)
    status = np.empty(lead, dtype=np.uint32)
    dp = C.POINTER(C.c_double)
    _check(_lib.load().ngd_mds_host(v.ctypes.data_as(dp), n_mat, n_ind, Kc, eig.ctypes.data_as(dp), vec.ctypes.data_as(dp),
                                    tot.ctypes.data_as(dp), status.ctypes.data_as(C.POINTER(C.c_uint32))))
    return eig, vec, tot, status


def win_cmp_max_vec():
    """the most vectors a comparison of windows takes (ngd_win_cmp_max_vec)"""
    return int(_lib.load().ngd_win_cmp_max_vec())


def win_cmp_slice(n_vec, n_cells):
    """cells per slice of the cell axis in the comparison of n_vec vectors of n_cells cells (ngd_win_cmp_slice)"""
    return int(_lib.load().ngd_win_cmp_slice(int(n_vec), int(n_cells)))


def win_cmp_host(values):
    """the comparison of windows in plain host arithmetic (ngd_win_cmp_host), the device form's twin: values
    float64[n_vec][n_cells] -> (mean float64[n_vec], gram float64[n_vec][n_vec], status uint32[n_vec])"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.ndim != 2:
        raise ValueError("values: expected [n_vec][n_cells]")
    W, P = v.shape
    mean = np.empty(W, dtype=np.float64)
    gram = np.empty((W, W), dtype=np.float64)
    status = np.empty(W, dtype=np.uint32)
    dp = C.POINTER(C.c_double)
    _check(_lib.load().ngd_win_cmp_host(v.ctypes.data_as(dp), W, P, mean.ctypes.data_as(dp), gram.ctypes.data_as(dp),
                                        status.ctypes.data_as(C.POINTER(C.c_uint32))))
    return mean, gram, status


def win_cmp_finish(mean, gram, status, n_cells):
    """the Mantel correlations and RMS differences of compared windows (ngd_win_cmp_finish): -> (cor float64[n_vec][n_vec],
    rms float64[n_vec][n_vec]); NaN wherever a status-0 vector is touched, cor NaN where a diagonal of gram is exactly 0"""
    m = np.ascontiguousarray(mean, dtype=np.float64)
    g = np.ascontiguousarray(gram, dtype=np.float64)
    st = np.ascontiguousarray(status, dtype=np.uint32)
    W = m.size
    if m.ndim != 1 or g.shape != (W, W) or st.shape != (W,):
        raise ValueError("expected mean [n_vec], gram [n_vec][n_vec], status [n_vec]")
    cor = np.empty((W, W), dtype=np.float64)
    rms = np.empty((W, W), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    _check(_lib.load().ngd_win_cmp_finish(m.ctypes.data_as(dp), g.ctypes.data_as(dp), st.ctypes.data_as(C.POINTER(C.c_uint32)), W,
                                          int(n_cells), cor.ctypes.data_as(dp), rms.ctypes.data_as(dp)))
    return cor, rms


def mds_coords(eig, vec):
    """the coordinates of eigenpairs (ngd_mds_coords): eig float64[..., K], vec float64[..., K, n] -> float64[..., n, K],
    vec[k][i] * sqrt(max(eig[k], 0))"""
    e = np.ascontiguousarray(eig, dtype=np.float64)
    v = np.ascontiguousarray(vec, dtype=np.float64)
    if v.ndim < 2 or e.shape != v.shape[:-1]:
        raise ValueError("eig, vec: expected [..., K] and [..., K, n]")
    lead, K, n = v.shape[:-2], v.shape[-2], v.shape[-1]
    out = np.empty(lead + (n, K), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    _check(_lib.load().ngd_mds_coords(e.ctypes.data_as(dp), v.ctypes.data_as(dp), int(np.prod(lead, dtype=np.int64)), n, K,
                                      out.ctypes.data_as(dp)))
    return out


def mds_align_host(eig, vec, status=None):
    """the replicates of every set rotated onto its matrix 0 in plain host arithmetic (ngd_mds_align_host), the device
    form's twin: eig float64[..., n_mat, K], vec float64[..., n_mat, K, n], status uint32[..., n_mat] (None: every matrix
    has status 1) -> (aligned float64[..., n_mat, K, n], fit float64[..., n_mat]); coordinates are vec[k][i] *
    sqrt(max(eig[k], 0)), matrix 0 stays as it is (fit 0), a matrix left out is NaN"""
    e = np.ascontiguousarray(eig, dtype=np.float64)
    v = np.ascontiguousarray(vec, dtype=np.float64)
    if v.ndim < 3 or e.shape != v.shape[:-1]:
        raise ValueError("eig, vec: expected [..., n_mat, K] and [..., n_mat, K, n]")
    lead, n_mat, K, n = v.shape[:-3], v.shape[-3], v.shape[-2], v.shape[-1]
    sp = None
    if status is not None:
        st = np.ascontiguousarray(status, dtype=np.uint32)
        if st.shape != lead + (n_mat,):
            raise ValueError("status: expected [..., n_mat]")
        sp = st.ctypes.data_as(C.POINTER(C.c_uint32))
    aligned = np.empty(v.shape, dtype=np.float64)
    fit = np.empty(lead + (n_mat,), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    _check(_lib.load().ngd_mds_align_host(e.ctypes.data_as(dp), v.ctypes.data_as(dp), sp, int(np.prod(lead, dtype=np.int64)), n_mat, n, K,
                                          aligned.ctypes.data_as(dp), fit.ctypes.data_as(dp)))
    return aligned, fit


def score_congruence(score):
    """the symmetric score matrix as three weighted squares, score = SUM_r d[r] c[r] c[r]^T (ngd_score_congruence: what
    ngd_config.single_image = 2 builds its one operand image from).  Returns (c [3][3], d [3])."""
    L = _lib.load()
    s = np.ascontiguousarray(score, dtype=np.float64).reshape(9)
    c, d = np.zeros(9), np.zeros(3)
    dp = C.POINTER(C.c_double)
    _check(L.ngd_score_congruence(s.ctypes.data_as(dp), c.ctypes.data_as(dp), d.ctypes.data_as(dp)))
    return c.reshape(3, 3), d


def format_matrix(dist, labels, n_threads=0):
    """The print block of one matrix (ngsDist.cpp:282-287) as bytes, from ngd_finish()'s pair-ordered output."""
    L = _lib.load()
    d = np.ascontiguousarray(dist, dtype=np.float64)
    n_ind = len(labels)
    if d.size != n_ind * (n_ind - 1) // 2:
        raise ValueError("dist must hold n_ind*(n_ind-1)/2 cells")
    lab = (C.c_char_p * n_ind)(*[x.encode() if isinstance(x, str) else x for x in labels])
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    cap = 32 + sum(len(x) + 1 for x in lab) + n_ind * n_ind * 16  # enough unless cells are huge
    while True:
        buf = C.create_string_buffer(cap)
        need = L.ngd_format_matrix(dp, n_ind, lab, buf, cap, int(n_threads))
        if need < 0:
            _check(int(need))
        if need <= cap:
            return buf.raw[:need]
        cap = int(need)


class Taus:
    """gsl_rng_taus as the reference seeds and draws it (ngsDist.cpp:179-180, :421-423)."""

    def __init__(self, seed):
        self._L = _lib.load()
        self._st = (C.c_uint32 * 3)()
        self._L.ngd_taus_seed(self._st, int(seed) & 0xFFFFFFFFFFFFFFFF)

    def get(self):
        return int(self._L.ngd_taus_get(self._st))

    def uniform(self):
        return float(self._L.ngd_taus_uniform(self._st))

    def block_map(self, n_blocks):
        m = np.empty(int(n_blocks), dtype=np.uint64)
        self._L.ngd_boot_block_map(self._st, int(n_blocks), m.ctypes.data_as(C.POINTER(C.c_uint64)))
        return m
