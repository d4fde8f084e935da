// ngsdist_host.cpp -- command-line host of the MI355X engine.
//
// Keeps the ngsDist command line (reference parse_args.cpp:54-80, defaults
// :6-37, checks :203-220), its input formats (read_data.cpp:13-116), its
// preparation of the array gen_dist() reads (ngsDist.cpp:165-174) and its
// output (ngsDist.cpp:282-287, "%.10f" cells joined by tabs), and hands the one
// hot block -- `for i1<i2: threadpool_add(gen_dist_slave)` + wait,
// ngsDist.cpp:244-269 -- to the engine through the C ABI of
// include/ngsdist_amd.h.  Written from scratch against that behaviour; it
// shares no code with the reference.
//
// Differences that are deliberate:
//  * binary input is streamed through in site chunks (read -> prepare ->
//    ngd_upload_sites), so the host never holds the n_ind x n_sites x 3 array;
//  * preparation (log / normalise / call / exp, all on the host's libm so cells
//    print identically) runs on --n_threads threads; it is per-element, so the
//    result does not depend on the thread count;
//  * bootstrap moves no data: the block map drawn from the reference's taus
//    stream is handed to ngd_run();
//  * a file name without a '.' is treated as binary instead of dereferencing
//    NULL (ngsDist.cpp:82);
//  * extra options: --n_gpus N (the SITE axis split over N devices of this node: every device reads and holds its own
//    range of sites and computes all pairs over it; the per-range sums are added -- byte-identical output for called
//    genotypes, <= 1e-12 relative otherwise), --device D (first device), --same_device (every range on --device: a
//    rehearsal on one GPU), --max_device_bytes B (device budget; a data set above it goes through in several ranges
//    per device), --kernel auto|stream|mfma|em_table|em_fast|em_faithful, --single_image / --two_images (--indep_geno on
//    the MFMA kernel: ngd_config.single_image = 2 / 3 -- ONE operand image in coordinates in which the score matrix is
//    diagonal + min(p0, p2) beside it: two thirds of the device memory per site, half the HBM reads, the same speed;
//    called genotypes print the same bytes, likelihood sums agree to 4e-17 per site and the pairs that is not enough
//    for, nearly identical individuals, are recomputed the two-operand way -- the engine's own choice above 384
//    individuals; or both images always),
//    --prep auto|host|device (where log/normalise/call/exp of a BINARY input run; auto =
//    device, except host when genotypes are called so that calls are decided by glibc),
//    --eager 0|1|2 (1, the default: on the EM path without bootstrap the full-data pass starts beside the load,
//    NGD_OPT_EAGER_FULL; 2: on the --indep_geno path too; 0: never), --stage piece_MiB,ring[,share_MiB[,drop]] (the load
//    pipeline's geometry, for measurements: tools/r6_stage_sweep.sh), --groups FILE (the group of every individual: <out>
//    holds the G x G table of mean distances within and between groups of every matrix, <out>.used the cells behind them;
//    one GPU, the whole data set resident), --boot_stats [--boot_ci X] (with --n_boot_rep or --win_boot_rep: the replicates
//    stay on the device, <out> holds the estimates and <out>.boot_mean / _sd / _lo / _hi / _used the replicates' summaries
//    per cell; one GPU, the whole data set resident), --nj (the neighbour-joining tree of every matrix, built on the device:
//    <out>.nwk holds one Newick line per matrix, <out> matrix 0 of every set and, with replicates, <out>.support.nwk matrix
//    0's tree with the number of replicate trees that share each of its branches; one GPU, the whole data set resident),
//    --mds K (classical MDS / principal coordinates of every matrix, computed on the device: <out>.mds holds one block per
//    matrix -- a line "eig" with the K largest eigenvalues of the double-centred matrix, a line "total" with the sum of all
//    eigenvalues and of the positive ones, a line per individual with its label and K coordinates, an empty line; fields
//    are separated by tabs and every number is printed as "%.10e", "nan" throughout for a matrix with a cell that is not
//    finite --, <out> matrix 0 of every set; one GPU, the whole data set resident), --mds_align [--mds_ci X] (with --mds K and
//    --n_boot_rep or --win_boot_rep: the replicates' coordinates are rotated onto matrix 0's on the device and summarised
//    there: <out>.mds holds matrix 0 of every set alone, <out>.mds_mean / _sd / _lo / _hi the replicates' statistics in the
//    same blocks without the "total" line, <out>.mds_fit per set the replicates that went in and every replicate's squared
//    distance from matrix 0 after the rotation), --win_cmp [--win_cmp_mds K] (with --win_size or --win_bp: the windows'
//    matrices are compared with one another on the device: <out>.win_cor holds the Mantel correlation of every pair of
//    windows and <out>.win_rms their root-mean-square difference, one line per window of W tab-separated "%.10e", "nan"
//    where undefined; <out>.win_cmp per window its number, mean distance, standard deviation of its distances and status;
//    <out>.win_mds, with --win_cmp_mds K, the classical MDS of the RMS table in the block format of <out>.mds; <out> and
//    <out>.windows are the run's without the flag);
//  * a binary file is mapped and copied into the engine's ring of pinned buffers by --n_threads (4..16) threads, the
//    copies to the device and the preparation kernel running behind; matrices are written by a thread of their own
//    while the next one is formatted; --verbose 2 ends with a `> phases [s]:` line (where the run's wall time went).
//
// Layout: options (Pars, parse_cmd_args), text helpers, the readers and the Loader; then what the run reads beside the
// genotypes (read_labels, read_positions, make_windows: WindowList), device_fit (one device or site ranges), the matrix
// output every mode prints through (Writer, MatrixOut::emit), the jobs the modes share (draw_window_maps, draw_job_maps,
// format_grown, for_window_groups) and one function per output mode -- site_range_matrices, trees, coordinates, aligned_coordinates, bootstrap_summaries,
// group_means, window_matrices, compared_windows, plain_matrices; main(), last, is the run's outline and picks one of them.
#include <fcntl.h>
#include <getopt.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <ctime>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../../include/ngsdist_amd.h"

// The engine's windowed entry point is referred to weakly: a host linked against an engine without it (a stub) still
// links, and --win_size then fails with a message.  ngd_window_ranges (host_util.cpp) is always there.
#pragma weak ngd_run_windows_dist
#pragma weak ngd_last_windows
#pragma weak ngd_run_windows_job_dist  // (--win_boot_rep)
#pragma weak ngd_run_windows_job_var_dist  // (--win_boot_rep under --win_bp: windows of unequal length)
// (--groups: the group means of every matrix, reduced on the device)
#pragma weak ngd_set_groups
#pragma weak ngd_run_job_groups
#pragma weak ngd_run_windows_groups
#pragma weak ngd_run_windows_job_var_groups
// (--boot_stats: the summaries over a set's replicates, reduced on the device)
#pragma weak ngd_boot_stats_max_rep
#pragma weak ngd_run_job_stats
#pragma weak ngd_run_windows_job_var_stats
#pragma weak ngd_run_job_groups_stats
#pragma weak ngd_run_windows_job_var_groups_stats
// (--nj: a neighbour-joining tree per matrix, built on the device)
#pragma weak ngd_nj_max_ind
#pragma weak ngd_run_job_nj
#pragma weak ngd_run_windows_nj
#pragma weak ngd_run_windows_job_var_nj
#pragma weak ngd_nj_support
#pragma weak ngd_nj_newick
// (--mds: the principal coordinates of every matrix, computed on the device; ngd_mds_max_dim and ngd_mds_coords are
// host_util.cpp's and always there)
#pragma weak ngd_mds_max_ind
#pragma weak ngd_run_job_mds
#pragma weak ngd_run_windows_mds
#pragma weak ngd_run_windows_job_var_mds
#pragma weak ngd_run_job_mds_align  // (--mds_align)
#pragma weak ngd_run_windows_job_var_mds_align
#pragma weak ngd_run_windows_cmp  // (--win_cmp: the windows' matrices compared with one another on the device)
#pragma weak ngd_win_cmp_finish
#pragma weak ngd_win_cmp_max_vec
#pragma weak ngd_last_em_exact  // (--em_exact: what the recheck noted and changed; the option itself goes through ngd_set_option)

static const char *kVersion = "ngsdist_amd 0.1 (ngsDist 1.0.10 command line)";
static const double kInf = 1e15;          // INF, gen_func.hpp:15
static const size_t kLineBuf = 500000;    // BUFF_LEN, gen_func.hpp:17

struct Pars {  // the reference's `params`, ngsDist.hpp:11-44
  const char *in_geno = nullptr;
  bool in_bin = false, in_probs = false, in_logscale = false;
  uint64_t n_ind = 0, n_sites = 0, tot_sites = 0;
  const char *in_labels = nullptr;
  bool in_labels_header = false;
  const char *in_pos = nullptr;
  bool in_pos_header = false;
  bool call_geno = false;
  double N_thresh = 0, call_thresh = 0;
  bool pairwise_del = false;
  double score[9] = {0, 0.5, 1, 0.5, 0, 0.5, 1, 0.5, 0};  // parse_args.cpp:25-27
  uint64_t evol_model = 1;
  bool indep_geno = false;
  uint64_t n_boot_rep = 0, boot_block_size = 1;
  const char *out = nullptr;
  unsigned n_threads = 1, verbose = 1, seed = 0;
  // engine placement (not in the reference)
  int n_gpus = 1, device = 0, kernel = NGD_KERNEL_AUTO;
  bool same_device = false;      // --same_device
  uint64_t max_device_bytes = 0; // --max_device_bytes (0 = 85 % of the device's free memory)
  bool single_image = false;     // --single_image
  bool two_images = false;       // --two_images
  int prep = 0;  // 0 auto (device unless genotypes are called), 1 host, 2 device
  unsigned stage_piece = 0, stage_ring = 0, stage_grain = 2, stage_drop = 1;  // --stage (0: the engine's defaults)
  int eager = 1;  // --eager 0|1|2: the full-data pass beside the load where the first engine call is that pass
  // --win_size / --win_step: one matrix per window of sites along the genome (not in the reference)
  bool win = false, win_step_set = false;
  uint64_t win_size = 0, win_step = 0;
  // --win_boot_rep: bootstrap replicates drawn INSIDE every window (blocks of --boot_block_size sites of the window, --seed):
  // per window what the reference prints for the cut-down file with --n_boot_rep.  Not --n_boot_rep, which resamples the genome.
  bool win_boot = false;
  uint64_t win_boot_rep = 0;
  // --win_bp / --win_bp_step / --win_min_sites: the same windows in coordinates -- window k of a chromosome covers the
  // positions [1 + k step, 1 + k step + size) of the positions file's second column, kept if it holds --win_min_sites sites.
  // Turns on --win_size's flow (win is set): its refusals, plans and files; --win_boot_rep draws per-window maps.
  bool win_bp = false, win_bp_step_set = false, win_min_sites_set = false;
  long long win_bp_size = 0, win_bp_step = 0, win_min_sites = 1;
  // --em_exact: on the EM path the full-data pass stops every (pair, site) at the reference's EM step (NGD_OPT_EM_EXACT: the
  // stops within rounding of the tolerance are rerun on the host).  Not in the reference.
  bool em_exact = false;
  // --em_exact_boot: the same, and allowed together with --n_boot_rep: every replicate's matrix is patched from the same
  // list, weighted by its block multiplicities (NGD_OPT_EM_EXACT = 2).  --em_exact itself keeps refusing replicates.
  bool em_exact_boot = false;
  // --em_exact_win: the same for the windows of --win_size, and for the replicates inside them with --win_boot_rep
  // (NGD_OPT_EM_EXACT = 1, or 2 with replicates, and NGD_OPT_EM_EXACT_WIN).  The two flags above keep refusing windows.
  bool em_exact_win = false;
  // --groups FILE: one line per individual, its first field the name of the individual's group (NA, - or an empty line: in
  // no group).  <out> then holds, per matrix, the G x G table of mean distances within and between groups -- the engine
  // reduces every matrix on the device (ngd_run_*_groups) -- and <out>.used the cells behind each mean.  Not in the reference.
  const char *in_groups = nullptr;
  // --boot_stats [--boot_ci X]: with --n_boot_rep R or --win_boot_rep R the replicates stay on the device, which reduces
  // every cell of a set (the run's, or a window's R + 1 matrices) to its estimate, the replicates' mean, standard deviation
  // and a percentile interval of coverage X (ngd_run_*_stats).  <out> holds matrix 0 of every set -- the run without
  // replicates --, <out>.boot_mean / .boot_sd / .boot_lo / .boot_hi the same blocks of the other statistics and
  // <out>.boot_used the finite replicates behind them.  With --groups the cells are the group pairs.  Not in the reference.
  bool boot_stats = false, boot_ci_set = false;
  double boot_ci = 0.95;
  // --nj: every matrix of the run -- the full data set and its --n_boot_rep replicates, or the windows and their
  // --win_boot_rep replicates -- leaves the engine as its neighbour-joining tree (ngd_run_*_nj): <out>.nwk holds one Newick
  // line per matrix in block order, <out> matrix 0 of every set (a plain run: the run without --nj) and, with replicates,
  // <out>.support.nwk matrix 0's tree of every set with its branches' support.  Not in the reference, whose README pipes
  // the matrices through fastme and RAxML for the same files.
  bool nj = false;
  // --mds K: every matrix of the run -- as for --nj -- leaves the engine as the top K eigenpairs of its double-centred form
  // and the two sums of its eigenvalues (ngd_run_*_mds): <out>.mds holds one block per matrix in block order -- "eig" and
  // its K eigenvalues, "total" and the two sums, a line per individual with its K coordinates vec * sqrt(max(eig, 0)), an
  // empty line; tabs between fields, numbers as "%.10e" --, <out> matrix 0 of every set (a plain run: the run without
  // --mds).  Not in the reference, whose users run R's cmdscale on <out>.
  bool mds = false;
  uint64_t mds_dim = 0;
  // --mds_align [--mds_ci X]: with --mds K and replicates, the replicates' coordinates are rotated onto matrix 0's
  // (orthogonal Procrustes) and summarised on the device (ngd_run_*_mds_align): <out>.mds holds matrix 0 of every set,
  // <out>.mds_mean / _sd / _lo / _hi the statistics of the aligned coordinates and of the eigenvalues, <out>.mds_fit per set
  // the replicates that went in and their fits.  Not in the reference, whose users run vegan::procrustes in a loop.
  bool mds_align = false, mds_ci_set = false;
  double mds_ci = 0.95;
  // --win_cmp: the windows of --win_size / --win_bp are compared with one another where their matrices lie
  // (ngd_run_windows_cmp): <out>.win_cor, <out>.win_rms and <out>.win_cmp beside the run's own <out> and <out>.windows;
  // --win_cmp_mds K: the classical MDS of the RMS table of the windows that were kept, on the host (ngd_mds_host):
  // <out>.win_mds.  Not in the reference
  bool win_cmp = false, win_cmp_mds = false;
  uint64_t win_cmp_dim = 0;
};

// --verbose 2: where the wall time of a run goes, as one line of name=seconds pairs at the end of the run (stderr; the
// reference prints nothing comparable).  A mark closes the phase that ran since the previous mark.
struct PhaseLog {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
  std::vector<std::pair<std::string, double>> phases;
  std::mutex mu;  // (--n_gpus: every device's thread loads its own ranges)
  void mark(const char *name) {
    std::lock_guard<std::mutex> lk(mu);
    const auto t = std::chrono::steady_clock::now();
    phases.emplace_back(name, std::chrono::duration<double>(t - last).count());
    last = t;
  }
  void add(const char *name, double secs) {  // a component measured elsewhere (not on the timeline)
    std::lock_guard<std::mutex> lk(mu);
    phases.emplace_back(name, secs);
  }
  void print() const {
    fprintf(stderr, "> phases [s]:");
    for (auto &ph : phases) fprintf(stderr, " %s=%.4f", ph.first.c_str(), ph.second);
    fprintf(stderr, " total_since_main=%.4f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
};
static PhaseLog g_phases;

// error(), gen_func.cpp:12-18: message, perror, exit(-1)
[[noreturn]] static void die(const char *func, const char *msg) {
  fflush(stdout);
  fprintf(stderr, "\n=====\nERROR: [%s] %s\n=====\n\n", func, msg);
  perror("\t");
  fflush(stderr);
  exit(-1);
}

static void die_engine(const char *func, int rc) {
  std::string m = std::string("engine error ") + std::to_string(rc) + ": " + ngd_last_error();
  die(func, m.c_str());
}

// One-image engines (--single_image, or the engine's own choice: include/ngsdist_amd.h ngd_config.single_image): what the
// fix-up pass of nearly identical pairs did in the last engine call.  Pairs it had to leave alone (more of them than its
// budget covers: a large data set of copies of one individual) keep an ABSOLUTE error bound -- far below what "%.10f"
// prints, but the user should know; said once.  --verbose 2: the pairs recomputed, every call.
static uint64_t g_exact_noted = 0, g_exact_changed = 0;  // --em_exact / --em_exact_boot / --em_exact_win: over every engine and call (site ranges add up)
static void report_fixup(ngd_engine *h, uint64_t verbose) {
  ngd_em_exact_info x;
  if (ngd_last_em_exact && ngd_last_em_exact(h, &x) == NGD_OK) {
    g_exact_noted += x.noted;
    g_exact_changed += x.changed;
  }
  ngd_fixup_info f;
  if (ngd_last_fixup(h, &f) != NGD_OK) return;
  static bool warned = false;
  if (f.skipped && !warned) {
    warned = true;
    fprintf(stderr, "WARNING: %lu pairs of nearly identical individuals keep the sums of the one-image pass (absolute error <= 4e-17 "
                    "per site, not 1e-9 relative): more of them than the recomputation's budget covers; --two_images holds "
                    "1e-9 relative on every pair.\n", (unsigned long)f.skipped);
  }
  if (verbose >= 2 && f.recomputed)
    fprintf(stderr, "> %lu pairs of nearly identical individuals recomputed with the two-operand arithmetic (%.2f ms)\n",
            (unsigned long)f.recomputed, f.ms);
}

static const char *kModelNames[] = {"Raw p-distance", "Log transf. p-distance", "JC69", "K80", "F81",
                                    "HKY85/F84", "TN93"};

static void parse_cmd_args(Pars &p, int argc, char **argv) {
  static struct option opts[] = {{"geno", required_argument, nullptr, 'g'},
                                 {"probs", no_argument, nullptr, 'p'},
                                 {"log_scale", no_argument, nullptr, 'l'},
                                 {"n_ind", required_argument, nullptr, 'n'},
                                 {"n_sites", required_argument, nullptr, 's'},
                                 {"tot_sites", required_argument, nullptr, 'S'},
                                 {"labels", required_argument, nullptr, 'L'},
                                 {"labelsH", required_argument, nullptr, 'H'},
                                 {"pos", required_argument, nullptr, 'a'},
                                 {"posH", required_argument, nullptr, 'A'},
                                 {"call_geno", no_argument, nullptr, 'c'},
                                 {"N_thresh", required_argument, nullptr, 'N'},
                                 {"call_thresh", required_argument, nullptr, 'C'},
                                 {"pairwise_del", no_argument, nullptr, 'D'},
                                 {"avg_nuc_dist", no_argument, nullptr, 'd'},
                                 {"evol_model", required_argument, nullptr, 'm'},
                                 {"indep_geno", no_argument, nullptr, 'I'},
                                 {"n_boot_rep", required_argument, nullptr, 'b'},
                                 {"boot_block_size", required_argument, nullptr, 'B'},
                                 {"out", required_argument, nullptr, 'o'},
                                 {"n_threads", required_argument, nullptr, 'x'},
                                 {"verbose", required_argument, nullptr, 'V'},
                                 {"seed", required_argument, nullptr, 'r'},
                                 {"n_gpus", required_argument, nullptr, 1001},
                                 {"same_device", no_argument, nullptr, 1005},
                                 {"max_device_bytes", required_argument, nullptr, 1006},
                                 {"single_image", no_argument, nullptr, 1007},
                                 {"two_images", no_argument, nullptr, 1008},
                                 {"device", required_argument, nullptr, 1002},
                                 {"kernel", required_argument, nullptr, 1003},
                                 {"prep", required_argument, nullptr, 1004},
                                 {"stage", required_argument, nullptr, 1009},
                                 {"eager", required_argument, nullptr, 1010},
                                 {"win_size", required_argument, nullptr, 1011},
                                 {"win_step", required_argument, nullptr, 1012},
                                 {"win_boot_rep", required_argument, nullptr, 1013},
                                 {"em_exact", no_argument, nullptr, 1014},
                                 {"em_exact_boot", no_argument, nullptr, 1015},
                                 {"em_exact_win", no_argument, nullptr, 1016},
                                 {"win_bp", required_argument, nullptr, 1017},
                                 {"win_bp_step", required_argument, nullptr, 1018},
                                 {"win_min_sites", required_argument, nullptr, 1019},
                                 {"groups", required_argument, nullptr, 1020},
                                 {"boot_stats", no_argument, nullptr, 1021},
                                 {"boot_ci", required_argument, nullptr, 1022},
                                 {"nj", no_argument, nullptr, 1023},
                                 {"mds", required_argument, nullptr, 1024},
                                 {"mds_align", no_argument, nullptr, 1025},
                                 {"mds_ci", required_argument, nullptr, 1026},
                                 {"win_cmp", no_argument, nullptr, 1027},
                                 {"win_cmp_mds", required_argument, nullptr, 1028},
                                 {nullptr, 0, nullptr, 0}};
  p.seed = (unsigned)time(nullptr);  // parse_args.cpp:35
  int c;
  while ((c = getopt_long_only(argc, argv, "g:pln:s:S:a:A:L:H:cN:C:Ddm:Ib:B:o:x:V:r:", opts, nullptr)) != -1) {
    switch (c) {
      case 'g': p.in_geno = optarg; break;
      case 'p': p.in_probs = true; break;
      case 'l': p.in_logscale = true; p.in_probs = true; break;  // --log_scale implies --probs
      case 'n': p.n_ind = (uint64_t)atol(optarg); break;
      case 's': p.n_sites = (uint64_t)atol(optarg); break;
      case 'S': p.tot_sites = (uint64_t)atol(optarg); break;
      case 'L': p.in_labels = optarg; p.in_labels_header = false; break;
      case 'H': p.in_labels = optarg; p.in_labels_header = true; break;
      case 'a': p.in_pos = optarg; p.in_pos_header = false; break;
      case 'A': p.in_pos = optarg; p.in_pos_header = true; break;
      case 'c': p.call_geno = true; break;
      case 'N': p.N_thresh = atof(optarg); p.call_geno = true; break;    // -N / -C imply --call_geno
      case 'C': p.call_thresh = atof(optarg); p.call_geno = true; break;
      case 'D': p.pairwise_del = true; break;
      case 'd': p.score[4] = 0.5; break;  // --avg_nuc_dist, parse_args.cpp:134-137
      case 'm': p.evol_model = (uint64_t)atol(optarg); break;
      case 'I': p.indep_geno = true; break;
      case 'b': p.n_boot_rep = (uint64_t)atol(optarg); break;
      case 'B': p.boot_block_size = (uint64_t)atol(optarg); break;
      case 'o': p.out = optarg; break;
      case 'x': p.n_threads = (unsigned)atoi(optarg); break;
      case 'V': p.verbose = (unsigned)atoi(optarg); break;
      case 'r': p.seed = (unsigned)atoi(optarg); break;
      case 1001: p.n_gpus = atoi(optarg); break;
      case 1005: p.same_device = true; break;
      case 1006: p.max_device_bytes = strtoull(optarg, nullptr, 10); break;
      case 1010: p.eager = atoi(optarg); break;
      case 1011: p.win = true; p.win_size = strtoull(optarg, nullptr, 10); break;
      case 1012: p.win_step_set = true; p.win_step = strtoull(optarg, nullptr, 10); break;
      case 1013: p.win_boot = true; p.win_boot_rep = strtoull(optarg, nullptr, 10); break;
      case 1014: p.em_exact = true; break;
      case 1015: p.em_exact_boot = true; break;
      case 1016: p.em_exact_win = true; break;
      case 1017: p.win_bp = true; p.win_bp_size = strtoll(optarg, nullptr, 10); break;
      case 1018: p.win_bp_step_set = true; p.win_bp_step = strtoll(optarg, nullptr, 10); break;
      case 1019: p.win_min_sites_set = true; p.win_min_sites = strtoll(optarg, nullptr, 10); break;
      case 1020: p.in_groups = optarg; break;
      case 1021: p.boot_stats = true; break;
      case 1022: p.boot_ci_set = true; p.boot_ci = atof(optarg); break;
      case 1023: p.nj = true; break;
      case 1024: {
        char *end = nullptr;
        p.mds = true;
        p.mds_dim = strtoull(optarg, &end, 10);
        if (end == optarg || *end || optarg[0] == '-') die(__FUNCTION__, "the number of dimensions (--mds K) must be a whole number!");
        break;
      }
      case 1025: p.mds_align = true; break;
      case 1026: p.mds_ci_set = true; p.mds_ci = atof(optarg); break;
      case 1027: p.win_cmp = true; break;
      case 1028: {
        char *end = nullptr;
        p.win_cmp_mds = true;
        p.win_cmp_dim = strtoull(optarg, &end, 10);
        if (end == optarg || *end || optarg[0] == '-') die(__FUNCTION__, "the number of dimensions (--win_cmp_mds K) must be a whole number!");
        break;
      }
      case 1009:  // --stage piece_MiB,ring[,copy share MiB[,drop pages 0|1]]: the load pipeline's geometry (measurement)
        if (sscanf(optarg, "%u,%u,%u,%u", &p.stage_piece, &p.stage_ring, &p.stage_grain, &p.stage_drop) < 2)
          die(__FUNCTION__, "--stage takes piece_MiB,ring[,share_MiB[,drop]]");
        break;
      case 1007: p.single_image = true; break;
      case 1008: p.two_images = true; break;
      case 1002: p.device = atoi(optarg); break;
      case 1003:
        if (!strcmp(optarg, "auto")) p.kernel = NGD_KERNEL_AUTO;
        else if (!strcmp(optarg, "stream")) p.kernel = NGD_KERNEL_STREAM;
        else if (!strcmp(optarg, "mfma")) p.kernel = NGD_KERNEL_MFMA;
        else if (!strcmp(optarg, "em_fast")) p.kernel = NGD_KERNEL_EM_FAST;
        else if (!strcmp(optarg, "em_faithful")) p.kernel = NGD_KERNEL_EM_FAITHFUL;
        else if (!strcmp(optarg, "em_table")) p.kernel = NGD_KERNEL_EM_TABLE;
        else die(__FUNCTION__, "unknown --kernel");
        break;
      case 1004:
        if (!strcmp(optarg, "auto")) p.prep = 0;
        else if (!strcmp(optarg, "host")) p.prep = 1;
        else if (!strcmp(optarg, "device")) p.prep = 2;
        else die(__FUNCTION__, "unknown --prep");
        break;
      default: exit(-1);
    }
  }
  if (p.verbose >= 1) {
    fprintf(stderr, "==> Input Arguments:\n");
    fprintf(stderr,
            "\tgeno: %s\n\tprobs: %s\n\tlog_scale: %s\n\tn_ind: %lu\n\tn_sites: %lu\n\ttot_sites: %lu\n"
            "\tlabels: %s (%s header)\n\tpositions: %s (%s header)\n\tcall_geno: %s\n\tN_thresh: %f\n"
            "\tcall_thresh: %f\n\tpairwise_del: %s\n\tavg_nuc_dist: %s\n\tevol_model: %s\n\tgeno_indep: %s\n"
            "\tn_boot_rep: %lu\n\tboot_block_size: %lu\n\tout: %s\n\tn_threads: %d\n\tverbose: %d\n\tseed: %d\n"
            "\tversion: %s\n\n",
            p.in_geno, p.in_probs ? "true" : "false", p.in_logscale ? "true" : "false", p.n_ind, p.n_sites,
            p.tot_sites, p.in_labels, p.in_labels_header ? "WITH" : "WITHOUT", p.in_pos,
            p.in_pos_header ? "WITH" : "WITHOUT", p.call_geno ? "true" : "false", p.N_thresh, p.call_thresh,
            p.pairwise_del ? "true" : "false", p.score[4] == 0.5 ? "true" : "false",
            p.evol_model <= 6 ? kModelNames[p.evol_model] : "?", p.indep_geno ? "true" : "false", p.n_boot_rep,
            p.boot_block_size, p.out, p.n_threads, p.verbose, p.seed, kVersion);
    if (p.win || p.win_step_set)
      fprintf(stderr, "\twin_size: %lu\n\twin_step: %lu\n\n", p.win_size, p.win_step_set ? p.win_step : p.win_size);
    if (p.win_bp || p.win_bp_step_set || p.win_min_sites_set)
      fprintf(stderr, "\twin_bp: %lld\n\twin_bp_step: %lld\n\twin_min_sites: %lld\n\n", p.win_bp_size,
              p.win_bp_step_set ? p.win_bp_step : p.win_bp_size, p.win_min_sites);
    if (p.win_boot) fprintf(stderr, "\twin_boot_rep: %lu\n\n", p.win_boot_rep);
    if (p.em_exact) fprintf(stderr, "\tem_exact: true\n\n");
    if (p.em_exact_boot) fprintf(stderr, "\tem_exact_boot: true\n\n");
    if (p.em_exact_win) fprintf(stderr, "\tem_exact_win: true\n\n");
    if (p.in_groups) fprintf(stderr, "\tgroups: %s\n\n", p.in_groups);
    if (p.boot_stats) fprintf(stderr, "\tboot_stats: true\n\tboot_ci: %f\n\n", p.boot_ci);
    if (p.nj) fprintf(stderr, "\tnj: true\n\n");
    if (p.mds) fprintf(stderr, "\tmds: %lu\n\n", (unsigned long)p.mds_dim);
    if (p.mds_align) fprintf(stderr, "\tmds_align: true\n\tmds_ci: %f\n\n", p.mds_ci);
    if (p.win_cmp) fprintf(stderr, "\twin_cmp: true\n\twin_cmp_mds: %lu\n\n", (unsigned long)p.win_cmp_dim);
  }
  if (p.verbose > 4)
    fprintf(stderr, "==> Verbose values greater than 4 for debugging purpose only. Expect large amounts of info on screen\n");
  // parse_args.cpp:203-220
  if (!p.in_geno) die(__FUNCTION__, "genotype input file (--geno) missing!");
  if (p.n_ind == 0) die(__FUNCTION__, "number of individuals (--n_ind) missing!");
  if (p.n_sites == 0) die(__FUNCTION__, "number of sites (--n_sites) missing!");
  if (p.tot_sites > 0 && p.pairwise_del)
    die(__FUNCTION__, "cannot specify total number of sites (--tot_sites) with pairwise deletion (--pairwise_del)!");
  if (p.call_geno && !p.in_probs) die(__FUNCTION__, "can only call genotypes from likelihoods/probabilities!");
  if (p.evol_model > 6) die(__FUNCTION__, "invalid correction method specified!");
  if (p.evol_model > 2 && !p.in_pos)
    die(__FUNCTION__, "use of more complex evolutionary models requires position information!");
  if (!p.out) die(__FUNCTION__, "output prefix (--out) missing!");
  if (p.n_threads < 1) die(__FUNCTION__, "number of threads cannot be less than 1!");
  if (p.n_gpus < 1) die(__FUNCTION__, "number of GPUs cannot be less than 1!");
  if (p.boot_block_size < 1) die(__FUNCTION__, "bootstrap block size cannot be less than 1!");
  if (p.win_bp && p.win) die(__FUNCTION__, "windows in base pairs (--win_bp) cannot be combined with windows in sites (--win_size)!");
  if (p.win_bp_step_set && !p.win_bp) die(__FUNCTION__, "window step in base pairs (--win_bp_step) requires a window size in base pairs (--win_bp)!");
  if (p.win_min_sites_set && !p.win_bp) die(__FUNCTION__, "minimum number of sites per window (--win_min_sites) requires a window size in base pairs (--win_bp)!");
  if (p.win_bp) {
    if (!p.win_bp_step_set) p.win_bp_step = p.win_bp_size;
    if (p.win_bp_size < 1) die(__FUNCTION__, "window size in base pairs (--win_bp) cannot be less than 1!");
    if (p.win_bp_step < 1) die(__FUNCTION__, "window step in base pairs (--win_bp_step) cannot be less than 1!");
    if (p.win_min_sites < 1) die(__FUNCTION__, "minimum number of sites per window (--win_min_sites) cannot be less than 1!");
    if (!p.in_pos) die(__FUNCTION__, "windows in base pairs (--win_bp) require a positions file (--pos / --posH)!");
    if (p.win_step_set) die(__FUNCTION__, "window step (--win_step) requires a window size (--win_size)!");
    p.win = true;  // from here on --win_size's flow, with its refusals
  }
  if (p.win_step_set && !p.win) die(__FUNCTION__, "window step (--win_step) requires a window size (--win_size)!");
  if (p.win_boot && !p.win) die(__FUNCTION__, "bootstrap replicates inside windows (--win_boot_rep) require a window size (--win_size)!");
  if (p.win_boot && p.n_boot_rep > 0)
    die(__FUNCTION__, "bootstrap replicates inside windows (--win_boot_rep) cannot be combined with bootstrap replicates of the whole data set (--n_boot_rep)!");
  if (p.win_boot && p.win_boot_rep >= (1ull << 31)) die(__FUNCTION__, "too many bootstrap replicates inside windows (--win_boot_rep)!");
  if (p.em_exact) {
    if (p.indep_geno || p.call_geno || !p.in_probs)  // (genotypes, given or called, go the --indep_geno way: ngsDist.cpp:55-65)
      die(__FUNCTION__, "the reference's EM stopping step (--em_exact) belongs to the EM path: not with --indep_geno / --call_geno or genotype input!");
    if (p.n_boot_rep > 0) die(__FUNCTION__, "the reference's EM stopping step (--em_exact) cannot be combined with bootstrap replicates (--n_boot_rep)!");
    if (p.win) die(__FUNCTION__, "the reference's EM stopping step (--em_exact) cannot be combined with windows (--win_size)!");
    p.eager = 0;  // (the pass started beside the load does not note)
  }
  if (p.em_exact_boot) {
    if (p.indep_geno || p.call_geno || !p.in_probs)
      die(__FUNCTION__, "the reference's EM stopping step (--em_exact_boot) belongs to the EM path: not with --indep_geno / --call_geno or genotype input!");
    if (p.win) die(__FUNCTION__, "the reference's EM stopping step (--em_exact_boot) cannot be combined with windows (--win_size)!");
    p.eager = 0;
  }
  if (p.em_exact_win) {  // (beside either flag above, that flag's own check has died already)
    if (p.indep_geno || p.call_geno || !p.in_probs)
      die(__FUNCTION__, "the reference's EM stopping step (--em_exact_win) belongs to the EM path: not with --indep_geno / --call_geno or genotype input!");
    if (!p.win) die(__FUNCTION__, "the reference's EM stopping step inside windows (--em_exact_win) needs windows (--win_size)!");
    if (p.win_bp && p.win_boot_rep)
      die(__FUNCTION__, "the reference's EM stopping step inside windows (--em_exact_win) serves plain windows in base pairs (--win_bp) only: not with --win_boot_rep!");
    p.eager = 0;
  }
  if (p.win) {
    if (!p.win_bp) {
      if (!p.win_step_set) p.win_step = p.win_size;
      if (p.win_size < 1) die(__FUNCTION__, "window size (--win_size) cannot be less than 1!");
      if (p.win_step < 1) die(__FUNCTION__, "window step (--win_step) cannot be less than 1!");
    }
    if (p.n_boot_rep > 0) die(__FUNCTION__, "windows (--win_size) cannot be combined with bootstrap replicates (--n_boot_rep)!");
    if (p.n_gpus > 1) die(__FUNCTION__, "windows (--win_size) are computed on one GPU (--n_gpus 1)!");
  }
  if (p.in_groups && p.n_gpus > 1) die(__FUNCTION__, "group means (--groups) are computed on one GPU (--n_gpus 1)!");
  if (p.boot_ci_set && !p.boot_stats) die(__FUNCTION__, "interval coverage (--boot_ci) requires bootstrap summaries (--boot_stats)!");
  if (p.boot_stats) {
    if (!(p.boot_ci > 0.0 && p.boot_ci < 1.0)) die(__FUNCTION__, "interval coverage (--boot_ci) must lie between 0 and 1!");
    if (p.n_boot_rep < 1 && p.win_boot_rep < 1)
      die(__FUNCTION__, "bootstrap summaries (--boot_stats) require bootstrap replicates (--n_boot_rep or --win_boot_rep)!");
    if (p.n_gpus > 1) die(__FUNCTION__, "bootstrap summaries (--boot_stats) are computed on one GPU (--n_gpus 1)!");
  }
  if (p.nj) {
    if (p.in_groups) die(__FUNCTION__, "neighbour-joining trees (--nj) cannot be combined with group means (--groups)!");
    if (p.boot_stats) die(__FUNCTION__, "neighbour-joining trees (--nj) cannot be combined with bootstrap summaries (--boot_stats)!");
    if (p.n_gpus > 1) die(__FUNCTION__, "neighbour-joining trees (--nj) are computed on one GPU (--n_gpus 1)!");
    if (p.n_ind < 3) die(__FUNCTION__, "neighbour-joining trees (--nj) need three individuals or more (--n_ind)!");
  }
  if (p.mds) {
    if (p.in_groups) die(__FUNCTION__, "classical MDS (--mds) cannot be combined with group means (--groups)!");
    if (p.boot_stats) die(__FUNCTION__, "classical MDS (--mds) cannot be combined with bootstrap summaries (--boot_stats)!");
    if (p.nj) die(__FUNCTION__, "classical MDS (--mds) cannot be combined with neighbour-joining trees (--nj)!");
    if (p.n_gpus > 1) die(__FUNCTION__, "classical MDS (--mds) is computed on one GPU (--n_gpus 1)!");
    if (p.n_ind < 3) die(__FUNCTION__, "classical MDS (--mds) needs three individuals or more (--n_ind)!");
    if (p.mds_dim < 1 || p.mds_dim > p.n_ind - 1 || p.mds_dim > ngd_mds_max_dim())
      die(__FUNCTION__, ("the number of dimensions (--mds K) must lie between 1 and min(n_ind - 1, " + std::to_string(ngd_mds_max_dim()) + ")!").c_str());
  }
  if (p.mds_ci_set && !p.mds_align) die(__FUNCTION__, "interval coverage (--mds_ci) requires aligned replicates (--mds_align)!");
  if (p.mds_align) {
    if (!p.mds) die(__FUNCTION__, "aligned replicates (--mds_align) require classical MDS (--mds K)!");
    if (!(p.mds_ci > 0.0 && p.mds_ci < 1.0)) die(__FUNCTION__, "interval coverage (--mds_ci) must lie between 0 and 1!");
    if (p.n_boot_rep < 1 && p.win_boot_rep < 1)
      die(__FUNCTION__, "aligned replicates (--mds_align) require bootstrap replicates (--n_boot_rep or --win_boot_rep)!");
  }
  if (p.win_cmp_mds && !p.win_cmp) die(__FUNCTION__, "the ordination of the windows (--win_cmp_mds) requires their comparison (--win_cmp)!");
  if (p.win_cmp) {
    if (!p.win) die(__FUNCTION__, "the comparison of windows (--win_cmp) requires windows (--win_size or --win_bp)!");
    if (p.win_boot_rep) die(__FUNCTION__, "the comparison of windows (--win_cmp) cannot be combined with bootstrap replicates inside windows (--win_boot_rep)!");
    if (p.in_groups) die(__FUNCTION__, "the comparison of windows (--win_cmp) cannot be combined with group means (--groups)!");
    if (p.boot_stats) die(__FUNCTION__, "the comparison of windows (--win_cmp) cannot be combined with bootstrap summaries (--boot_stats)!");
    if (p.nj) die(__FUNCTION__, "the comparison of windows (--win_cmp) cannot be combined with neighbour-joining trees (--nj)!");
    if (p.mds) die(__FUNCTION__, "the comparison of windows (--win_cmp) cannot be combined with classical MDS (--mds)!");
    if (p.n_gpus > 1) die(__FUNCTION__, "the comparison of windows (--win_cmp) is computed on one GPU (--n_gpus 1)!");
    if (p.n_ind < 2) die(__FUNCTION__, "the comparison of windows (--win_cmp) needs two individuals or more (--n_ind)!");
    if (p.win_cmp_mds && (p.win_cmp_dim < 1 || p.win_cmp_dim > ngd_mds_max_dim()))
      die(__FUNCTION__, ("the number of dimensions (--win_cmp_mds K) must lie between 1 and min(windows kept - 1, " + std::to_string(ngd_mds_max_dim()) + ")!").c_str());
  }
}

// ---------------------------------------------------------------------------
// text helpers with the reference's semantics
// ---------------------------------------------------------------------------
static gzFile open_gz(const char *name, const char *mode) {  // open_gzfile, gen_func.cpp:208-223
  gzFile fh = strcmp(name, "-") == 0 ? gzdopen(fileno(stdin), mode) : gzopen(name, mode);
  if (fh && gzbuffer(fh, 1 << 20) < 0) return nullptr;
  return fh;
}

static void chomp(char *s) {  // gen_func.cpp:192-199: drops ONE trailing \n or \r
  size_t n = strlen(s);
  if (n && (s[n - 1] == '\n' || s[n - 1] == '\r')) s[n - 1] = '\0';
}

// read_file(), gen_func.cpp:238-283: lines, minus empty ones and ones starting
// with '#', minus `offset` leading ones; a final line without '\n' is lost to
// the gzeof() check exactly as there.
static std::vector<std::string> read_lines(const char *path, uint64_t offset) {
  gzFile fh = open_gz(path, "r");
  if (!fh) die("read_file", "cannot open file!");
  std::vector<std::string> out;
  std::vector<char> buf(kLineBuf);
  for (;;) {
    buf[0] = '\0';
    gzgets(fh, buf.data(), (int)buf.size());
    if (gzeof(fh)) break;
    chomp(buf.data());
    if (buf[0] == '\0' || buf[0] == '#') continue;
    if (offset) { offset--; continue; }
    out.emplace_back(buf.data());
  }
  gzclose(fh);
  return out;
}

// --groups: every line of the file (empty ones too: an individual in no group), its first field the group's name; groups
// are numbered in order of first appearance, "NA", "-" and an empty field are -1
static void read_groups(const char *path, std::vector<int32_t> &group_of, std::vector<std::string> &names) {
  gzFile fh = open_gz(path, "r");
  if (!fh) die("read_file", "cannot open file!");
  std::unordered_map<std::string, int32_t> ids;
  std::vector<char> buf(kLineBuf);
  while (gzgets(fh, buf.data(), (int)buf.size())) {
    std::string l(buf.data());
    while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
    l.resize(std::min(l.size(), l.find_first_of("\t ")));
    if (l.empty() || l == "NA" || l == "-") {
      group_of.push_back(-1);
      continue;
    }
    const auto ins = ids.emplace(l, (int32_t)names.size());
    if (ins.second) names.push_back(l);
    group_of.push_back(ins.first->second);
  }
  gzclose(fh);
}

// --groups: the print block of one matrix's group means, in the layout of a distance matrix's block (ngsDist.cpp:282-287):
// "\n<G>\n", then per group its name and G cells "\t%.10f" -- the within-group mean on the diagonal, "nan" where no cell
// was finite --; `cnt` takes the same block with the numbers of cells behind the means.  mean / used: [n_gp], a <= b
static void format_groups(const std::vector<std::string> &names, const double *mean, const uint64_t *used, std::string &txt,
                          std::string &cnt) {
  const uint32_t G = (uint32_t)names.size();
  char cell[64];
  txt += "\n" + std::to_string(G) + "\n";
  cnt += "\n" + std::to_string(G) + "\n";
  for (uint32_t a = 0; a < G; a++) {
    txt += names[a];
    cnt += names[a];
    for (uint32_t b = 0; b < G; b++) {
      const uint64_t lo = std::min(a, b), hi = std::max(a, b);
      const uint64_t gp = lo * G - lo * (lo ? lo - 1 : 0) / 2 + (hi - lo);  // (ngd_group_pair_index)
      snprintf(cell, sizeof(cell), "\t%.10f", mean[gp]);
      txt += cell;
      snprintf(cell, sizeof(cell), "\t%lu", (unsigned long)used[gp]);
      cnt += cell;
    }
    txt += "\n";
    cnt += "\n";
  }
}

// strtod for the common spelling [-+]digits[.digits][e[-+]digits], exactly: up to 19 significant digits are
// gathered in an integer; when it is below 2^53 and the decimal exponent within +-22 the value is one
// correctly rounded multiplication or division by an exact power of ten (Clinger's fast path), which is what a
// correctly rounding strtod returns too.  Anything else (more digits, nan, inf, hex, junk) goes to strtod.
static inline bool fast_strtod(const char *s, size_t len, double *out) {
  static const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  const char *p = s, *end = s + len;
  bool neg = false;
  if (p < end && (*p == '-' || *p == '+')) neg = *p++ == '-';
  uint64_t m = 0;
  int nd = 0, e10 = 0;
  bool any = false;
  for (; p < end && *p >= '0' && *p <= '9'; p++) {
    any = true;
    if (m || *p != '0') { if (++nd > 19) return false; m = m * 10 + (uint64_t)(*p - '0'); }
  }
  if (p < end && *p == '.') {
    for (p++; p < end && *p >= '0' && *p <= '9'; p++) {
      any = true;
      if (m || *p != '0') { if (++nd > 19) return false; m = m * 10 + (uint64_t)(*p - '0'); }
      e10--;
    }
  }
  if (!any) return false;
  if (p < end && (*p == 'e' || *p == 'E')) {
    p++;
    bool eneg = false;
    if (p < end && (*p == '-' || *p == '+')) eneg = *p++ == '-';
    if (p >= end) return false;
    int ex = 0;
    for (; p < end && *p >= '0' && *p <= '9'; p++) { ex = ex * 10 + (*p - '0'); if (ex > 10000) return false; }
    e10 += eneg ? -ex : ex;
  }
  if (p != end) return false;
  if (m >> 53) return false;
  double v = (double)m;
  if (m == 0) v = 0.0;
  else if (e10 > 0) { if (e10 > 22) return false; v *= p10[e10]; }
  else if (e10 < 0) { if (e10 < -22) return false; v /= p10[-e10]; }
  *out = neg ? -v : v;
  return true;
}

// split(str, " \t", double**), gen_func.cpp:390-417: tokens between separators,
// empty tokens dropped, tokens that strtod does not consume entirely dropped.
static void split_doubles(char *line, const char *sep, std::vector<double> &out) {
  out.clear();
  char *s = line;
  while (s && *s) {
    size_t len = strcspn(s, sep);
    char *next = s[len] ? s + len + 1 : nullptr;
    s[len] = '\0';
    if (len) {
      double v;
      if (fast_strtod(s, len, &v)) out.push_back(v);
      else {
        char *end;
        v = strtod(s, &end);
        if (!*end) out.push_back(v);
      }
    }
    s = next;
  }
}

// ---------------------------------------------------------------------------
// preparation of one (individual, site): read_data.cpp:37-45 / :84-98, then
// ngsDist.cpp:165-174.  Same operation order and libm calls as the reference.
// ---------------------------------------------------------------------------
static inline void post_prob3(double *l) {  // gen_func.cpp:920-932 with logsum :135-151
  double M = l[0];
  for (int i = 1; i < 3; i++) M = (l[i] >= M ? l[i] : M);
  double norm;
  if (M == -INFINITY) {
    norm = -INFINITY;
  } else {
    double sum = 0;
    for (int i = 0; i < 3; i++) sum += exp(l[i] - M);
    norm = log(sum) + M;
  }
  for (int i = 0; i < 3; i++) l[i] -= norm;
}

static inline void call_geno3(double *l, double N_thresh, double call_thresh) {  // gen_func.cpp:886-914
  if (N_thresh > call_thresh) die("call_geno", "missing data threshold must be smaller than calling genotype threshold!");
  int max_pos = 0, min_pos = 0;
  double mx = -INFINITY, mn = INFINITY;
  for (int g = 0; g < 3; g++) if (l[g] > mx) { mx = l[g]; max_pos = g; }
  for (int g = 0; g < 3; g++) if (l[g] < mn) { mn = l[g]; min_pos = g; }
  double max_pp = exp(l[max_pos]);
  if (l[min_pos] == l[max_pos]) max_pp = -1;
  if (max_pp < N_thresh) for (int g = 0; g < 3; g++) l[g] = log((double)1 / 3);
  if (max_pp >= call_thresh) {
    for (int g = 0; g < 3; g++) l[g] = -kInf;
    l[max_pos] = log(1);
  }
}

static inline void finish_prep(const Pars &p, double *l) {  // ngsDist.cpp:165-174
  if (p.call_geno) call_geno3(l, p.N_thresh, p.call_thresh);
  for (int g = 0; g < 3; g++) l[g] = exp(l[g]);
}

// binary element; returns false on NaN (read_data.cpp:42-45)
static inline bool prep_binary(const Pars &p, bool in_logscale, double *l) {
  if (!in_logscale)
    for (int g = 0; g < 3; g++) {
      l[g] = log(l[g]);
      if (l[g] == -INFINITY) l[g] = -kInf;  // conv_space, gen_func.cpp:123-130
    }
  post_prob3(l);
  if (std::isnan(l[0]) || std::isnan(l[1]) || std::isnan(l[2])) return false;
  finish_prep(p, l);
  return true;
}

template <typename F>
static void parallel_for(unsigned n_threads, uint64_t n, uint64_t min_n, F fn) {
  if (n_threads <= 1 || n < min_n || n < 2) { fn(0, n); return; }
  std::vector<std::thread> th;
  uint64_t per = (n + n_threads - 1) / n_threads;
  for (unsigned t = 0; t < n_threads; t++) {
    uint64_t lo = t * per, hi = std::min(n, lo + per);
    if (lo >= hi) break;
    th.emplace_back(fn, lo, hi);
  }
  for (auto &t : th) t.join();
}

// The two parallel phases of a text group (tokenise, then parse + prepare) run a hundred times per load: their threads
// are kept ([measured] 541 MB of GL text, 16 threads: 0.29 s in the two phases with a thread spawned per share and call,
// of which 0.11 s is the work).  One user at a time (the text loader's thread); shares are handed out dynamically.
struct TextPool {
  std::mutex m;
  std::condition_variable cv_go, cv_done;
  std::vector<std::thread> workers;
  std::function<void(uint64_t, uint64_t)> job;
  uint64_t n = 0, per = 1, next = 0, done = 0, generation = 0;
  bool quit = false;
  explicit TextPool(unsigned n_threads) {
    for (unsigned t = 1; t < n_threads; t++)
      workers.emplace_back([this]() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
          cv_go.wait(lk, [&] { return quit || generation != seen; });
          if (quit) return;
          seen = generation;
          work(lk);
        }
      });
  }
  ~TextPool() {
    { std::lock_guard<std::mutex> lk(m); quit = true; }
    cv_go.notify_all();
    for (auto &w : workers) w.join();
  }
  void work(std::unique_lock<std::mutex> &lk) {  // takes shares until none is left; lk held on entry and exit
    while (next < n) {
      const uint64_t lo = next, hi = std::min(n, lo + per);
      next = hi;
      lk.unlock();
      job(lo, hi);
      lk.lock();
      done += hi - lo;
      if (done == n) cv_done.notify_all();
    }
  }
  template <typename F>
  void run(uint64_t count, F fn) {
    if (workers.empty() || count < 2) { fn(0, count); return; }
    std::unique_lock<std::mutex> lk(m);
    job = fn;
    n = count;
    per = std::max<uint64_t>(1, count / (4 * (workers.size() + 1)));
    next = done = 0;
    generation++;
    cv_go.notify_all();
    work(lk);
    cv_done.wait(lk, [&] { return done == n; });
    n = 0;
  }
};

// ---------------------------------------------------------------------------
// BGZF text input (the blocked gzip that bgzip / htslib / ANGSD write: a series of gzip members of at most 64 KB, each
// with its compressed size in a 'BC' extra field).  zlib's gzread -- the reference's reader, gen_func.cpp:208-223 --
// inflates such a file like any other .gz, one member after the other on one thread; the members being independent, here
// they are inflated on --n_threads threads, a few hundred at a time, CRCs checked as gzread checks them.  gets() has
// gzgets' semantics, so everything downstream (line splitting, headers, premature / missing EOF) is the same code.
struct BgzfText {
  int fd = -1;
  uint64_t size = 0, off = 0;  // file size; offset of the first block not yet inflated
  std::vector<unsigned char> comp;
  std::vector<char> text;      // the inflated blocks of the current batch
  size_t cur = 0;
  bool hit_eof = false, bad = false;
  unsigned n_threads = 1;
  static constexpr size_t kBatch = 16u << 20;  // compressed bytes per batch

  // size of the block at q (at least 18 bytes readable), 0 if it is not a BGZF block
  static uint32_t block_size(const unsigned char *q, size_t avail) {
    if (avail < 18 || q[0] != 0x1f || q[1] != 0x8b || q[2] != 8 || !(q[3] & 4)) return 0;
    const uint32_t xlen = q[10] | (uint32_t)q[11] << 8;
    if (12 + (size_t)xlen > avail) return 0;
    for (uint32_t x = 0; x + 4 <= xlen;) {
      const unsigned char *f = q + 12 + x;
      const uint32_t slen = f[2] | (uint32_t)f[3] << 8;
      if (f[0] == 'B' && f[1] == 'C' && slen == 2 && x + 6 <= xlen) return (f[4] | (uint32_t)f[5] << 8) + 1u;
      x += 4 + slen;
    }
    return 0;
  }
  static BgzfText *open_if_bgzf(const char *path, unsigned n_threads) {
    int fd = open(path, O_RDONLY);
    if (fd < 0) return nullptr;
    struct stat st;
    unsigned char head[64];
    const ssize_t n = pread(fd, head, sizeof(head), 0);
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || n < 18 || block_size(head, (size_t)n) < 26) {
      close(fd);
      return nullptr;
    }
    BgzfText *b = new BgzfText();
    b->fd = fd;
    b->size = (uint64_t)st.st_size;
    b->n_threads = std::max(1u, n_threads);
    return b;
  }
  ~BgzfText() { if (fd >= 0) close(fd); }

  // inflates the next batch of blocks into `text`; false when the file is used up (or damaged: bad)
  bool fill() {
    text.clear();
    cur = 0;
    while (text.empty()) {
      if (off >= size || bad) return false;
      const size_t want = (size_t)std::min<uint64_t>(kBatch, size - off);
      comp.resize(want);
      size_t got = 0;
      while (got < want) {
        const ssize_t r = pread(fd, comp.data() + got, want - got, (off_t)(off + got));
        if (r <= 0) { bad = true; return false; }
        got += (size_t)r;
      }
      struct Blk { size_t in, in_len, out; uint32_t isize, crc; };
      std::vector<Blk> blks;
      size_t q = 0, total = 0;
      while (q + 18 <= want) {
        const uint32_t bs = block_size(comp.data() + q, want - q);
        if (!bs) { bad = true; return false; }  // not a BGZF block where one must start
        if (q + bs > want) break;               // the batch ends inside this block: it opens the next batch
        const uint32_t xlen = comp[q + 10] | (uint32_t)comp[q + 11] << 8;
        if (bs < 20 + xlen) { bad = true; return false; }
        const unsigned char *t = comp.data() + q + bs - 8;
        Blk b;
        b.in = q + 12 + xlen;
        b.in_len = bs - 20 - xlen;
        b.crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        b.isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (b.isize > (1u << 16)) { bad = true; return false; }
        b.out = total;
        total += b.isize;
        blks.push_back(b);
        q += bs;
      }
      if (q == 0) { bad = true; return false; }  // a block larger than what is left of the file
      text.resize(total);
      std::atomic<int> err{0};
      parallel_for(n_threads, blks.size(), 8, [&](uint64_t lo, uint64_t hi) {
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, -15) != Z_OK) { err = 1; return; }
        for (uint64_t k = lo; k < hi && !err; k++) {
          const Blk &b = blks[k];
          if (!b.isize) continue;
          if (inflateReset(&zs) != Z_OK) { err = 1; break; }  // (one state per thread, re-armed for every block)
          zs.next_in = comp.data() + b.in;
          zs.avail_in = (uInt)b.in_len;
          zs.next_out = (Bytef *)text.data() + b.out;
          zs.avail_out = b.isize;
          const int rc = inflate(&zs, Z_FINISH);
          if (rc != Z_STREAM_END || zs.avail_out != 0 ||
              crc32(crc32(0L, Z_NULL, 0), (const Bytef *)text.data() + b.out, b.isize) != b.crc)
            err = 1;
        }
        inflateEnd(&zs);
      });
      if (err) { bad = true; text.clear(); return false; }
      off += q;
    }
    return true;
  }
  char *gets(char *buf, int len) {  // gzgets: up to len-1 characters, through the first newline
    int w = 0;
    while (w < len - 1) {
      if (cur == text.size() && !fill()) { hit_eof = true; break; }
      const char *src = text.data() + cur;
      const size_t want = std::min(text.size() - cur, (size_t)(len - 1 - w));
      const char *nl = (const char *)memchr(src, '\n', want);
      const size_t take = nl ? (size_t)(nl - src) + 1 : want;
      memcpy(buf + w, src, take);
      w += (int)take;
      cur += take;
      if (nl) break;
    }
    if (!w) return nullptr;
    buf[w] = '\0';
    return buf;
  }
  // The next line as gzgets(buf, max_chars + 1) + chomp() would deliver it (a longer line comes in pieces, ONE trailing
  // \n or \r is dropped), copied once, straight out of the inflated batch.
  bool next_line(std::string &out, size_t max_chars) {
    out.clear();
    bool any = false;
    while (out.size() < max_chars) {
      if (cur == text.size() && !fill()) { hit_eof = true; break; }
      const char *src = text.data() + cur;
      const size_t want = std::min(text.size() - cur, max_chars - out.size());
      const char *nl = (const char *)memchr(src, '\n', want);
      const size_t take = nl ? (size_t)(nl - src) + 1 : want;
      out.append(src, take);
      cur += take;
      any = true;
      if (nl) break;
    }
    if (!any) return false;
    const size_t z = out.find('\0');  // what strlen() in chomp() and the std::string made of the C string would see
    if (z != std::string::npos) out.resize(z);
    if (!out.empty() && (out.back() == '\n' || out.back() == '\r')) out.pop_back();
    return true;
  }
  bool eof() const { return hit_eof && !bad; }
};

// ---------------------------------------------------------------------------
// one engine, destroyed with its scope
struct Engine {
  ngd_engine *h = nullptr;
  Engine() = default;
  Engine(const Engine &) = delete;
  Engine &operator=(const Engine &) = delete;
  void upload_sites(const double *p, uint64_t s0, uint64_t n) {
    int rc = ngd_upload_sites(h, p, s0, n);
    if (rc) die_engine("upload", rc);
  }
  void commit() {
    int rc = ngd_commit(h);
    if (rc == NGD_E_NAN) die("read_geno", "NaN found! Is the file format correct?");
    if (rc) die_engine("commit", rc);
  }
  // The run's LAST engine is not taken apart before the process exits: its device memory goes back to the driver with the
  // process ([measured, round 6] cfg 3: unmapping and releasing 34 GB of mapped pieces is 26 ms of a 0.75 s command, of which
  // the exit itself takes back 8).  Builds under AddressSanitizer destroy it all the same (the leak checker's business).
  bool leave_to_exit = false;
  ~Engine() {
#if defined(__SANITIZE_ADDRESS__)
    leave_to_exit = false;
#endif
    if (h && !leave_to_exit) ngd_destroy(h);
  }
};

// read_geno(), read_data.cpp:13-116, fused with the preparation and the upload.  The input is consumed front to
// back in one or more parts (ranges of sites: one per device, or several when the data set is larger than the
// devices): load() puts the next n_part sites into an engine as its sites 0 .. n_part-1 and commits them.  A plain
// binary file can also be entered at any site (first_site), so that every device's thread reads its own ranges.
struct Loader {
  const Pars &p;
  gzFile fh = nullptr;
  std::unique_ptr<BgzfText> bg;  // text input that turned out to be BGZF: inflated on several threads instead of by fh
  char *text_gets(char *buf, int len) { return bg ? bg->gets(buf, len) : gzgets(fh, buf, len); }
  bool text_eof() { return bg ? bg->eof() : gzeof(fh) != 0; }
  int raw_fd = -1;
  uint64_t raw_off = 0, raw_size = 0;
  uint64_t done = 0;  // sites of the whole input consumed by earlier parts
  bool eof = false;
  explicit Loader(const Pars &pars, uint64_t first_site = 0);
  bool seekable() const { return raw_fd >= 0; }
  void load(Engine &eng, uint64_t n_part, bool last_part);
  void finish(bool check_eof = true);
};

Loader::Loader(const Pars &pars, uint64_t first_site) : p(pars) {
  fh = open_gz(p.in_geno, p.in_bin ? "rb" : "r");
  if (!fh) die("read_geno", "cannot open GENO file!");
  if (!p.in_bin && strcmp(p.in_geno, "-") != 0 && p.n_threads > 1) {  // (on one thread gzread does the same job)
    bg.reset(BgzfText::open_if_bgzf(p.in_geno, p.n_threads));
    if (bg && p.verbose >= 2) fprintf(stderr, "> BGZF input: blocks are inflated on %u thread(s)\n", bg->n_threads);
  }
  // A binary GL file that is a plain regular file (the usual case; gzread would only copy it through) is read
  // with pread() on several threads straight into the destination: one thread moves ~12 GB/s out of the page
  // cache, which is less than the copy to the device and the preparation kernel take.
  if (p.in_bin && strcmp(p.in_geno, "-") != 0) {
    struct stat st;
    int fd = open(p.in_geno, O_RDONLY);
    unsigned char magic[2] = {0, 0};
    if (fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && pread(fd, magic, 2, 0) >= 0 &&
        !(magic[0] == 0x1f && magic[1] == 0x8b)) {
      raw_fd = fd;
      raw_size = (uint64_t)st.st_size;
      raw_off = first_site * p.n_ind * 24;
      done = first_site;
    } else if (fd >= 0) {
      close(fd);
    }
  }
}

void Loader::load(Engine &eng, uint64_t n_part, bool last_part) {
  const uint64_t n_ind = p.n_ind, n_sites = n_part;
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(n_sites, (64ull << 20) / (n_ind * 24)));
  bool in_logscale = p.in_logscale;
  const bool device_prep = p.in_bin && (p.prep == 2 || (p.prep == 0 && !p.call_geno));
  std::vector<double> buf(device_prep ? 0 : chunk * n_ind * 3);
  // (12, not 16: with the engine's own threads 16 copying threads overrun a CPU quota of 16 and the whole process is
  // throttled for a few ms every 100 ms -- [measured] gaps of 2-7 ms between copies at 100-ms intervals; 8-20 threads load
  // cfg 3 in the same 0.51-0.53 s, the copy engine being the pace)
  const unsigned n_io = std::min(12u, std::max(4u, p.n_threads));
  auto read_exact = [&](double *dst, uint64_t bytes) {
    if (raw_fd >= 0) {
      if (raw_off + bytes > raw_size) die("read_geno", "GENO file at premature EOF. Check GENO file and number of sites!");
      std::atomic<bool> bad{false};
      parallel_for(n_io, bytes, 8u << 20, [&](uint64_t lo, uint64_t hi) {
        while (lo < hi) {
          ssize_t r = pread(raw_fd, (char *)dst + lo, hi - lo, (off_t)(raw_off + lo));
          if (r <= 0) { bad = true; return; }
          lo += (uint64_t)r;
        }
      });
      if (bad) die("read_geno", "cannot read binary GENO file. Check GENO file and number of sites!");
      raw_off += bytes;
      return;
    }
    uint64_t got = 0;
    while (got < bytes) {
      int r = gzread(fh, (char *)dst + got, (unsigned)std::min<uint64_t>(bytes - got, 1u << 30));
      if (r <= 0) break;
      got += (uint64_t)r;
    }
    if (got != bytes) {
      if (gzeof(fh)) die("read_geno", "GENO file at premature EOF. Check GENO file and number of sites!");
      die("read_geno", "cannot read binary GENO file. Check GENO file and number of sites!");
    }
  };
  if (p.in_bin && device_prep) {
    // Straight into the engine's ring of pinned buffers; the copies to the device and the preparation kernel overlap the
    // filling of the next buffers.  A regular file is MAPPED and its pages copied by a few kept threads: [measured, round
    // 6, tools/host_read_pipeline, 8.6 GB in the page cache / in tmpfs] pread() on 16 threads moves 116 GB/s alone but
    // 27-47 GB/s while the copy engine reads host memory beside it; memcpy() out of a mapping 55-57 GB/s = the link's
    // 57.6 (first touch of the mapping's pages included).  Handing the mapping itself to the copy engine (no host copy at
    // all) works but pins pages at 16-50 GB/s, and is not used.  (A file truncated by someone else during the run is a
    // SIGBUS here, where pread would have reported a premature EOF.)
    // The pages a thread has copied it takes out of the page table again at once (MADV_DONTNEED on a shared file mapping
    // drops the translations, nothing else): left to one munmap() at the end -- or to the kernel at exit -- the 6 million
    // 4-KB translations of 24 GB cost 0.3-0.5 s of ONE core ([measured] cfg 3: load 0.89 s, the copies themselves 0.50 s);
    // a window mapped and unmapped per piece instead makes the copies three times slower (0.72-1.6 s).
    const char *map = nullptr;
    void *map_base = nullptr;
    uint64_t map_len = 0;
    const uint64_t pg = (uint64_t)sysconf(_SC_PAGESIZE);
    if (raw_fd >= 0) {
      if (raw_off + n_sites * n_ind * 24 > raw_size) die("read_geno", "GENO file at premature EOF. Check GENO file and number of sites!");
      const uint64_t lo = raw_off / pg * pg;
      map_len = raw_off + n_sites * n_ind * 24 - lo;
      void *m = mmap(nullptr, map_len, PROT_READ, MAP_SHARED, raw_fd, (off_t)lo);
      if (m != MAP_FAILED) { map_base = m; map = (const char *)m - lo; }  // (map + file offset = that byte; else: pread as before)
    }
    const bool mapped = map != nullptr;
    std::unique_ptr<TextPool> pool;
    if (mapped) pool.reset(new TextPool(n_io));
    auto copy_mapped = [&](double *dst, uint64_t bytes) {
      const uint64_t grain = (uint64_t)std::max(1u, p.stage_grain) << 20, n_g = (bytes + grain - 1) / grain;
      const char *src = map + raw_off;
      pool->run(n_g, [&](uint64_t g0, uint64_t g1) {
        const uint64_t b0 = g0 * grain, b1 = std::min(bytes, g1 * grain);
        memcpy((char *)dst + b0, src + b0, b1 - b0);
        // whole pages inside [b0, b1): a page shared with a neighbouring share stays (its owner may not have read it yet)
        const uint64_t a0 = ((uint64_t)(uintptr_t)(src + b0) + pg - 1) / pg * pg, a1 = (uint64_t)(uintptr_t)(src + b1) / pg * pg;
        if (a1 > a0 && p.stage_drop) madvise((void *)(uintptr_t)a0, a1 - a0, MADV_DONTNEED);
      });
      raw_off += bytes;
    };
    ngd_prep pr;
    pr.in_logscale = in_logscale; pr.call_geno = p.call_geno; pr.N_thresh = p.N_thresh; pr.call_thresh = p.call_thresh;
    double t_acq = 0, t_read = 0, t_sub = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double>(b - a).count();
    };
    for (uint64_t s0 = 0; s0 < n_sites;) {
      double *pin; uint64_t cap;
      auto t0 = now();
      int rc = ngd_stage_acquire(eng.h, &pin, &cap);
      if (rc) die_engine("ngd_stage_acquire", rc);
      const uint64_t n = std::min(cap, n_sites - s0);
      auto t1 = now();
      if (mapped) copy_mapped(pin, n * n_ind * 24);
      else read_exact(pin, n * n_ind * 24);
      auto t2 = now();
      t_acq += secs(t0, t1); t_read += secs(t1, t2);
      auto t3 = now();
      rc = ngd_stage_submit(eng.h, s0, n, &pr);
      if (rc) die_engine("ngd_stage_submit", rc);
      t_sub += secs(t3, now());
      s0 += n;
    }
    if (p.verbose >= 2)
      fprintf(stderr, "> staged load: waiting for a free pinned buffer %.3f s, reading %.3f s (%s), submitting %.3f s\n", t_acq,
              t_read, mapped ? "memcpy out of mapped windows of the file, on several threads" : "gzread", t_sub);
    if (map_base) {
      // (the mapping's pages are gone already; what is left are its page-table pages, 12 000 of them for 24 GB: ~9 ms
      // of one core, beside the distances instead of before them)
      void *mb = map_base;
      const uint64_t ml = map_len;
      std::thread([mb, ml]() { munmap(mb, ml); }).detach();
    }
    g_phases.add("of_load_wait_buffer", t_acq);
    g_phases.add("of_load_read", t_read);
    g_phases.add("of_load_submit", t_sub);
  } else if (p.in_bin) {
    for (uint64_t s0 = 0; s0 < n_sites; s0 += chunk) {
      const uint64_t n = std::min(chunk, n_sites - s0);
      read_exact(buf.data(), n * n_ind * 24);
      std::atomic<bool> bad{false};
      parallel_for(p.n_threads, n * n_ind, 4096, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t e = lo; e < hi; e++)
          if (!prep_binary(p, in_logscale, &buf[3 * e])) bad = true;
      });
      if (bad) die("read_geno", "NaN found! Is the file format correct?");
      eng.upload_sites(buf.data(), s0, n);
    }
  } else {
    // Text: decompression and line splitting are sequential; tokenising, number parsing and the
    // per-(individual, site) preparation of a group of lines run on --n_threads threads.  Which lines are
    // sites (empty line = site at its -INF fill; line without numbers, or a short FIRST line = header) is
    // settled in file order between the two parallel phases, so errors and messages come in the reference's order.
    const uint64_t n_geno = p.in_probs ? 3 : 1;
    const uint64_t need = n_ind * n_geno;
    std::vector<char> line(std::max<size_t>(kLineBuf, need * 32 + 4096));
    const uint64_t group = std::max<uint64_t>(1, std::min<uint64_t>(chunk, 1024));
    std::vector<std::string> lines, ahead;
    std::vector<std::vector<double>> toks(group);
    std::vector<int64_t> slot(group);  // site slot within the group, or -1
    uint64_t s = 0;
    // up to `max_lines` lines of the stream (decompression + line splitting: the sequential part of a text load)
    // (*hit_end: the stream ended before max_lines were read)
    auto read_lines_into = [&](std::vector<std::string> &out, uint64_t max_lines, bool *hit_end) {
      out.clear();
      *hit_end = false;
      if (bg) {
        std::string one;
        while (out.size() < max_lines) {
          if (!bg->next_line(one, line.size() - 1)) { *hit_end = true; break; }
          out.emplace_back(std::move(one));
          one.clear();  // (moved from: valid but unspecified)
        }
        return;
      }
      while (out.size() < max_lines) {
        if (text_gets(line.data(), (int)line.size()) == nullptr) { *hit_end = true; break; }
        chomp(line.data());
        out.emplace_back(line.data());
      }
    };
    TextPool pool(p.n_threads);
    bool have_ahead = false, end_ahead = false;
    double t_first = 0, t_work = 0, t_up = 0, t_join = 0;  // --verbose 2: where a text load spends its time
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
    while (s < n_sites) {
      if (have_ahead) {
        lines.swap(ahead);
        eof = end_ahead;
        have_ahead = false;
      } else {
        // a little read-ahead for header lines -- in the last part only: lines past a part belong to the next one
        const auto t0 = now();
        read_lines_into(lines, std::min<uint64_t>(group, n_sites - s + (last_part ? 64 : 0)), &eof);
        t_first += secs(t0);
      }
      const auto t_w0 = now();
      // The NEXT group is decompressed by a reader thread while this one is tokenised, parsed and uploaded.  It may
      // take only lines that belong to this part whatever this group turns out to hold: at least n_sites - s - (lines
      // of this group) sites are still to come after it.
      std::thread reader;
      {
        const uint64_t sure = n_sites - s > lines.size() ? n_sites - s - lines.size() : 0;
        const uint64_t next_max = std::min<uint64_t>(group, sure + (last_part && sure ? 64 : 0));
        if (next_max && !eof && !lines.empty()) {
          reader = std::thread([&, next_max]() { read_lines_into(ahead, next_max, &end_ahead); });
          have_ahead = true;
        }
      }
      struct Joiner {
        std::thread &t;
        double &acc;
        ~Joiner() {
          const auto t0 = std::chrono::steady_clock::now();
          if (t.joinable()) t.join();
          acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
      } joiner{reader, t_join};
      if (lines.empty()) {
        if (text_eof()) die("read_geno", "GENO file at premature EOF. Check GENO file and number of sites!");
        die("read_geno", "cannot read GZip GENO file. Check GENO file and number of sites!");
      }
      pool.run(lines.size(), [&](uint64_t lo, uint64_t hi) {
        for (uint64_t k = lo; k < hi; k++)
          if (lines[k].empty()) toks[k].clear();
          else split_doubles(&lines[k][0], " \t", toks[k]);
      });
      uint64_t filled = 0;
      for (uint64_t k = 0; k < lines.size(); k++) {
        slot[k] = -1;
        if (s + filled == n_sites)  // anything after the last site: the reference stops reading before it
          die("read_geno", "GENO file not at EOF. Check GENO file and number of sites!");
        if (!lines[k].empty()) {
          if (toks[k].empty() || (done + s + filled == 0 && toks[k].size() < need)) {  // header
            fprintf(stderr, "> Header found! Skipping line...\n");
            continue;
          }
          if (toks[k].size() < need) die("read_geno", "wrong GENO file format. Less fields than expected!");
        }
        slot[k] = (int64_t)filled++;
      }
      std::atomic<int> bad_geno{0};
      pool.run(lines.size(), [&](uint64_t lo, uint64_t hi) {
        for (uint64_t k = lo; k < hi; k++) {
          if (slot[k] < 0) continue;
          double *dst = &buf[(uint64_t)slot[k] * n_ind * 3];
          if (lines[k].empty()) {
            // empty line: the site keeps its -INF fill (read_data.cpp:21,58-59)
            for (uint64_t i = 0; i < n_ind; i++) {
              double *l = dst + 3 * i;
              l[0] = l[1] = l[2] = -kInf;
              finish_prep(p, l);
            }
            continue;
          }
          const double *ptr = toks[k].data() + (toks[k].size() - need);  // last n_ind*n_geno columns
          for (uint64_t i = 0; i < n_ind; i++) {
            double *l = dst + 3 * i;
            if (p.in_probs) {
              for (int g = 0; g < 3; g++) l[g] = in_logscale ? ptr[3 * i + g] : log(ptr[3 * i + g]);
            } else {
              l[0] = l[1] = l[2] = -kInf;
              int g = (int)ptr[i];
              if (g >= 0) {
                if (g > 2) { bad_geno = 1; g = 2; }
                l[g] = log(1);
              } else {
                l[0] = l[1] = l[2] = log((double)1 / 3);
              }
            }
            post_prob3(l);
            finish_prep(p, l);
          }
        }
      });
      if (bad_geno) die("read_geno", "wrong GENO file format. Genotypes must be coded as {-1,0,1,2} !");
      t_work += secs(t_w0);
      const auto t_u0 = now();
      if (filled) eng.upload_sites(buf.data(), s, filled);
      t_up += secs(t_u0);
      s += filled;
      if (eof && s < n_sites) die("read_geno", "GENO file at premature EOF. Check GENO file and number of sites!");
    }
    if (p.verbose >= 2)
      fprintf(stderr, "> text load: first group read %.3f s, tokenise + parse + prepare %.3f s, uploads %.3f s, waiting for the "
              "reader thread (inflate + line split of the next group) %.3f s\n", t_first, t_work, t_up, t_join);
  }
  done += n_part;
  {
    const auto t_c = std::chrono::steady_clock::now();
    eng.commit();
    g_phases.add("of_load_commit", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_c).count());
  }
}

void Loader::finish(bool check_eof) {
  if (raw_fd >= 0) {
    if (check_eof && raw_off != raw_size) die("read_geno", "GENO file not at EOF. Check GENO file and number of sites!");
    close(raw_fd);
  } else {
    char one[2];
    if (bg) {
      if (bg->gets(one, 2) != nullptr || !bg->eof())
        die("read_geno", bg->bad ? "cannot read GZip GENO file. Check GENO file and number of sites!"
                                 : "GENO file not at EOF. Check GENO file and number of sites!");
    } else {
    gzread(fh, one, 1);
    if (!gzeof(fh)) die("read_geno", "GENO file not at EOF. Check GENO file and number of sites!");
    }
  }
  gzclose(fh);
}

// ---------------------------------------------------------------------------
// The run.  main(), at the end of the file, is its outline.  Before it, in this order: what the run reads besides the
// genotypes (labels, groups, positions, the window list), whether the data set fits one device, the matrix output every
// mode prints through, the jobs several modes share (block maps, the loop over groups of windows), and one function per
// output mode.  The bracketed name of an error message is part of the program's output: the messages below keep the two
// names they are known by.
// ---------------------------------------------------------------------------
namespace {

const char *const kMain = "main", *const kLambda = "operator()";

void engine_ok(const char *call, int rc) { if (rc) die_engine(call, rc); }

double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// ngsDist.cpp:55-65 (which algorithm) and :73-95 (which input format)
void input_decisions(Pars &p) {
  if (!p.in_probs && !p.indep_geno) {
    fprintf(stderr, "==> Using faster algorithm (assuming independence of genotypes) since input are genotypes!\n");
    p.indep_geno = true;
  } else if (p.call_geno && !p.indep_geno) {
    fprintf(stderr, "==> Using faster algorithm (assuming independence of genotypes) since calling genotypes!\n");
    p.indep_geno = true;
  } else if (p.indep_geno && p.verbose >= 1) {
    fprintf(stderr, "==> Using faster algorithm (assuming independence of genotypes)!\n");
  }
  if (strcmp(p.in_geno, "-") == 0) {
    if (p.verbose >= 1) fprintf(stderr, "==> Reading from STDIN (BINARY)\n");
    p.in_bin = true;
  } else {
    struct stat st;
    if (stat(p.in_geno, &st) != 0) die(kMain, "cannot check GENO file size!");
    const char *dot = strrchr(p.in_geno, '.');
    if (dot && strcmp(dot, ".gz") == 0) {
      if (p.verbose >= 1) fprintf(stderr, "==> GZIP input file (never BINARY)\n");
      p.in_bin = false;
    } else {
      if (p.verbose >= 1) fprintf(stderr, "==> BINARY input file\n");
      p.in_bin = true;
      p.in_probs = true;
      if (p.n_sites != (uint64_t)st.st_size / sizeof(double) / p.n_ind / 3)
        die(kMain, "invalid/corrupt genotype input file!");
    }
  }
  if (p.evol_model > 2) {  // gen_dist() would error() on the first pair, ngsDist.cpp:387-398
    static const char *msg[] = {"K80 model not yet supported", "F81 model not yet supported",
                                "HKY85 model not yet supported", "TN93 model not yet supported"};
    die("gen_dist", msg[p.evol_model - 3]);
  }
}

// labels, ngsDist.cpp:103-125
std::vector<std::string> read_labels(const Pars &p) {
  std::vector<std::string> labels;
  if (p.in_labels) {
    if (p.verbose >= 1) fprintf(stderr, "==> Reading labels\n");
    labels = read_lines(p.in_labels, p.in_labels_header ? 1 : 0);
    if (labels.size() != p.n_ind) die(kMain, "invalid LABELS file!");
    for (auto &l : labels) l.resize(std::min(l.size(), l.find('\t')));  // (the first field)
  } else {
    for (uint64_t i = 0; i < p.n_ind; i++) labels.push_back("Ind_" + std::to_string(i));
  }
  if (p.verbose >= 4) for (auto &l : labels) fprintf(stderr, "%s\n", l.c_str());
  return labels;
}

// what --boot_stats, --nj and --mds need of the engine and of the job
void check_summaries_and_trees(const Pars &p) {
  if (p.boot_stats) {
    if (!ngd_boot_stats_max_rep || !ngd_run_job_stats || !ngd_run_windows_job_var_stats || !ngd_run_job_groups_stats ||
        !ngd_run_windows_job_var_groups_stats)
      die(kMain, "this build of the engine has no bootstrap summaries (--boot_stats)!");
    if (std::max<uint64_t>(p.n_boot_rep, p.win_boot_rep) > ngd_boot_stats_max_rep())
      die(kMain, "too many bootstrap replicates for bootstrap summaries (--boot_stats): a cell's replicates stay in on-chip memory!");
  }
  if (p.nj) {
    if (!ngd_nj_max_ind || !ngd_run_job_nj || !ngd_run_windows_nj || !ngd_run_windows_job_var_nj || !ngd_nj_support || !ngd_nj_newick)
      die(kMain, "this build of the engine has no neighbour-joining trees (--nj)!");
    if (p.n_ind > ngd_nj_max_ind())
      die(kMain, "too many individuals for neighbour-joining trees (--nj): a matrix's row sums stay in on-chip memory!");
  }
  if (p.mds) {
    if (!ngd_mds_max_ind || !ngd_run_job_mds || !ngd_run_windows_mds || !ngd_run_windows_job_var_mds)
      die(kMain, "this build of the engine has no classical MDS (--mds)!");
    if (p.n_ind > ngd_mds_max_ind())
      die(kMain, "too many individuals for classical MDS (--mds): a matrix's tridiagonal form stays in on-chip memory!");
  }
  if (p.mds_align) {
    if (!ngd_boot_stats_max_rep || !ngd_run_job_mds_align || !ngd_run_windows_job_var_mds_align)
      die(kMain, "this build of the engine has no aligned replicates (--mds_align)!");
    if (std::max<uint64_t>(p.n_boot_rep, p.win_boot_rep) > ngd_boot_stats_max_rep())
      die(kMain, "too many bootstrap replicates for aligned replicates (--mds_align): a cell's replicates stay in on-chip memory!");
  }
  if (p.win_cmp && (!ngd_run_windows_cmp || !ngd_win_cmp_finish || !ngd_win_cmp_max_vec))
    die(kMain, "this build of the engine has no comparison of windows (--win_cmp): not linked!");
}

// The windows of --win_size / --win_bp, and what the positions file says about the sites they hold.
struct WindowList {
  std::vector<uint64_t> lo, hi, bp_start;  // per window: its sites [lo, hi) and (--win_bp) its first coordinate
  std::vector<uint32_t> chrom;             // per site: its chromosome's number (empty without a positions file)
  std::vector<std::string> pos_txt;        // per site: its position as the file spells it
  std::vector<uint64_t> pos;               // --win_bp: the coordinates as numbers
  std::unordered_map<uint32_t, std::string> chr_name;
  uint64_t size() const { return lo.size(); }
  // as the progress lines call the window
  std::string name(uint64_t w) const { return std::to_string(w) + " [" + std::to_string(lo[w]) + ", " + std::to_string(hi[w]) + ")"; }
  // <out>.windows: where each window lies
  void write_file(const std::string &path, const Pars &p) const {
    FILE *wf = fopen(path.c_str(), "w");
    if (!wf) die(kLambda, "cannot open windows output file!");
    fprintf(wf, p.win_bp ? "window\tchr\tstart\tend\tfirst_site\tn_sites\twin_start\twin_end\n" : "window\tchr\tstart\tend\tfirst_site\tn_sites\n");
    for (uint64_t w = 0; w < size(); w++) {
      const uint64_t l = lo[w], h = hi[w];
      if (chrom.empty()) fprintf(wf, "%lu\t.\t%lu\t%lu\t%lu\t%lu", w, l + 1, h, l, h - l);
      else fprintf(wf, "%lu\t%s\t%s\t%s\t%lu\t%lu", w, chr_name.at(chrom[l]).c_str(), pos_txt[l].c_str(), pos_txt[h - 1].c_str(), l, h - l);
      // (--win_bp, which has the positions: + the window's own coordinates, inclusive: 1 + k T and k T + B)
      if (p.win_bp) fprintf(wf, "\t%lu\t%lu", bp_start[w], bp_start[w] + (uint64_t)p.win_bp_size - 1);
      fputc('\n', wf);
    }
    if (fclose(wf) != 0) die(kLambda, "cannot write windows output file!");
  }
};

// positions: validated, never used (models 3-6 are unimplemented), ngsDist.cpp:133-149 -- except for the chromosomes
// and coordinates of --win_size's windows
void read_positions(const Pars &p, WindowList &win) {
  if (p.verbose >= 1) fprintf(stderr, "==> Reading positions file\n");
  std::vector<std::string> pos = read_lines(p.in_pos, p.in_pos_header ? 1 : 0);
  uint64_t n_fields = 0;
  for (auto &l : pos) {
    uint64_t n = 1 + (uint64_t)std::count(l.begin(), l.end(), '\t');
    if (!l.empty() && l.back() == '\t') n--;  // no trailing empty field (_strtok, gen_func.cpp:305-322)
    if (n_fields == 0) n_fields = n;
    if (n != n_fields) die("read_split", "invalid number of fields in file!");
  }
  if (pos.size() != p.n_sites || n_fields < 2) die(kMain, "invalid POS file!");
  if (!p.win) return;
  // fields 1 (chromosome) and 2 (position) of every site: the windows' chromosomes and coordinates
  std::unordered_map<std::string, uint32_t> ids;
  win.chrom.resize(p.n_sites);
  win.pos_txt.resize(p.n_sites);
  win.pos.resize(p.win_bp ? p.n_sites : 0);
  for (uint64_t s = 0; s < p.n_sites; s++) {
    const std::string &l = pos[s];
    const size_t t1 = l.find('\t'), t2 = l.find('\t', t1 + 1);
    const std::string chr = l.substr(0, t1);
    win.chrom[s] = ids.emplace(chr, (uint32_t)ids.size()).first->second;
    win.pos_txt[s] = l.substr(t1 + 1, t2 == std::string::npos ? std::string::npos : t2 - t1 - 1);
    if (s == 0 || win.chrom[s] != win.chrom[s - 1]) win.chr_name.emplace(win.chrom[s], chr);
    if (!p.win_bp) continue;
    // --win_bp: whole numbers from 1 (below 2^62: ngd_window_ranges_bp) that do not descend inside a chromosome
    const std::string &t = win.pos_txt[s];
    const bool digits = !t.empty() && t.size() <= 18 && t.find_first_not_of("0123456789") == std::string::npos;
    win.pos[s] = digits ? strtoull(t.c_str(), nullptr, 10) : 0;
    if (!win.pos[s]) die(kMain, "invalid position in POS file: windows in base pairs (--win_bp) need whole numbers from 1!");
    if (s && win.chrom[s] == win.chrom[s - 1] && win.pos[s] < win.pos[s - 1])
      die(kMain, "positions descend inside a chromosome of the POS file: windows in base pairs (--win_bp) need them in ascending order!");
  }
}

// the windows (--win_size / --win_step, or --win_bp's in coordinates): the list the Python package makes too (host_util.cpp
// ngd_window_ranges, ngd_window_ranges_bp), and whether the engine has the entry points the plain windowed run goes through
void make_windows(const Pars &p, WindowList &win) {
  const uint64_t B = (uint64_t)p.win_bp_size, T = (uint64_t)p.win_bp_step, M = (uint64_t)p.win_min_sites;
  const uint32_t *ids = win.chrom.empty() ? nullptr : win.chrom.data();
  // both calls: first the number of windows, then the windows
  auto ranges = [&](uint64_t n) {
    return p.win_bp ? ngd_window_ranges_bp(ids, win.pos.data(), p.n_sites, B, T, M, win.lo.data(), win.hi.data(), win.bp_start.data(), n)
                    : ngd_window_ranges(ids, p.n_sites, p.win_size, p.win_step, win.lo.data(), win.hi.data(), n);
  };
  const int64_t n_win = ranges(0);
  if (n_win < 0) die(kMain, "positions file not grouped by chromosome!");
  if (n_win == 0)
    die(kMain, p.win_bp ? "no window is kept (--win_min_sites larger than every window's number of sites)!"
                        : "no window fits the data set (--win_size larger than every chromosome)!");
  win.lo.resize((size_t)n_win);
  win.hi.resize((size_t)n_win);
  if (p.win_bp) win.bp_start.resize((size_t)n_win);
  ranges((uint64_t)n_win);
  if (!p.in_groups && !p.boot_stats && !p.nj && !p.mds) {  // (--groups, --boot_stats, --nj, --mds: their own entry points, checked before)
    if (!ngd_run_windows_dist) die(kMain, "this build of the engine has no windows along the genome (--win_size)!");
    if (p.win_boot_rep && (p.win_bp ? !ngd_run_windows_job_var_dist : !ngd_run_windows_job_dist))
      die(kMain, p.win_bp ? "this build of the engine has no bootstrap replicates inside windows of unequal length (--win_bp with --win_boot_rep)!"
                          : "this build of the engine has no bootstrap replicates inside windows (--win_boot_rep)!");
  }
  if (p.verbose >= 1 && p.win_bp)
    fprintf(stderr, "==> %lu windows of %lu bp every %lu bp\n", (unsigned long)n_win, (unsigned long)B, (unsigned long)T);
  else if (p.verbose >= 1)
    fprintf(stderr, "==> %lu windows of %lu sites every %lu sites\n", (unsigned long)n_win, p.win_size, p.win_step);
}

// Does the data set fit ONE device?  Resident bytes per site: both operand images (one on the EM path, the
// individual-major copy for the streaming kernel), masks and bootstrap weights; plus slabs and results.  If it
// does and one device is asked for, one engine runs the whole job (ngd_run_job).  Otherwise gen_dist()'s sums are
// split along the SITE axis (include/ngsdist_amd.h "Site sharding"): ranges of sites, each read, held and computed
// by one device -- side by side on --n_gpus devices, one after the other where the devices are too small -- and
// the per-range (sum, cnt) are added.
struct DeviceFit {
  uint64_t per_site, fixed, budget;  // bytes: resident per site, needed whatever the sites, that a device may hold
  bool in_parts;                     // the job goes through in ranges of sites
};
DeviceFit device_fit(const Pars &p, uint64_t n_comb, uint64_t dev_free) {
  const uint64_t n_pad = (p.n_ind + 127) / 128 * 128;
  const bool mfma_path = p.indep_geno && p.kernel != NGD_KERNEL_STREAM;
  // (one image + the fix-up pass's side array, 24 n_pad + 8 n_ind: --single_image, or the engine's own choice above 384
  // padded individuals -- ngd_config.single_image = 0; this program's score matrices are the reference's two)
  const bool one_image = mfma_path && !p.two_images && (p.single_image || n_pad > 384);
  const uint64_t per_site = (p.kernel == NGD_KERNEL_STREAM ? 24 * p.n_ind
                             : one_image ? 24 * n_pad + 8 * p.n_ind : (mfma_path ? 48 : 24) * n_pad) +
                            (p.pairwise_del ? p.n_ind / 8 + 1 : 0) + 40;
  const uint64_t n_t = n_pad / 128, n_slabs = std::max<uint64_t>(8, std::min<uint64_t>(256, 8192 / (n_t * (n_t + 1) / 2)));
  const uint64_t fixed = n_slabs * n_pad * n_pad * 8 + n_comb * 64 + (512ull << 20);
  if (p.same_device) dev_free /= (uint64_t)p.n_gpus;  // the rehearsal's ranges share one device
  const uint64_t budget = p.max_device_bytes ? p.max_device_bytes : dev_free / 100 * 85;
  return {per_site, fixed, budget, p.n_gpus > 1 || fixed + per_site * p.n_sites > budget};
}

// an engine for n_sites_part sites on the run's dev_index-th device; eager_ranges: the job goes through in site ranges
void make_engine(const Pars &p, Engine &eng, uint64_t n_sites_part, int dev_index, bool eager_ranges) {
  ngd_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.n_ind = p.n_ind;
  cfg.n_sites = n_sites_part;
  memcpy(cfg.score, p.score, sizeof(cfg.score));
  cfg.pairwise_del = p.pairwise_del;
  cfg.indep_geno = p.indep_geno;
  cfg.device = p.same_device ? p.device : p.device + dev_index;
  cfg.kernel = p.kernel;
  // (the MFMA kernel on one operand image, on two, or -- 0 -- as the engine chooses; nothing to the other kernels)
  cfg.single_image = p.single_image ? 2 : p.two_images ? 3 : 0;
  engine_ok("ngd_create", ngd_create(&cfg, &eng.h));
  auto set = [&](int option, uint64_t value) { engine_ok("ngd_set_option", ngd_set_option(eng.h, option, value)); };
  // the first engine call after the load is the plain full-data pass (no bootstrap; or site ranges, whose engines always
  // begin with it): on the EM path, where that pass is several times the load, it starts beside the load
  // (NGD_OPT_EAGER_FULL: [measured] cfg 4 2.96 -> 2.78 s end to end; --eager 0 switches it off, --eager 2 also takes it
  // for --indep_geno, where a 46 ms pass beside a 0.5 s load gains nothing measurable)
  if (p.eager && (!p.indep_geno || p.eager >= 2) && (p.n_boot_rep == 0 || eager_ranges) && !p.win) set(NGD_OPT_EAGER_FULL, 1);
  if (p.em_exact || p.em_exact_boot) set(NGD_OPT_EM_EXACT, p.em_exact_boot ? 2 : 1);
  if (p.em_exact_win) {
    set(NGD_OPT_EM_EXACT, p.win_boot_rep ? 2 : 1);
    set(NGD_OPT_EM_EXACT_WIN, 1);
  }
  if (p.stage_piece) set(NGD_OPT_STAGE_PIECE_MIB, p.stage_piece);
  if (p.stage_ring) set(NGD_OPT_STAGE_RING, p.stage_ring);
}

// Text of unknown length: format(buffer, its size) returns the bytes the text takes (negative: it cannot be made) and
// writes it if it fits; where it does not, the buffer grows to that size once and the text is formatted again.
template <typename F>
int64_t format_grown(std::vector<char> &buf, F format) {
  int64_t need = format(buf.data(), buf.size());
  if (need > (int64_t)buf.size()) {
    buf.resize((size_t)need);
    need = format(buf.data(), buf.size());
  }
  return need;
}

// The thread that writes <out>: one piece of text at a time, in the order handed in.
struct Writer {
  FILE *fh = nullptr;
  std::mutex m;
  std::condition_variable cv;
  const char *data = nullptr;
  size_t len = 0;
  bool quit = false, failed = false, busy = false;
  std::thread th;
  void start(FILE *f) {
    fh = f;
    th = std::thread([this]() {
      std::unique_lock<std::mutex> lk(m);
      for (;;) {
        cv.wait(lk, [&] { return quit || data; });
        if (!data) return;
        const char *d = data;
        const size_t n = len;
        lk.unlock();
        const bool ok = fwrite(d, 1, n, fh) == n;
        lk.lock();
        if (!ok) failed = true;
        data = nullptr;
        busy = false;
        cv.notify_all();
      }
    });
  }
  void wait_idle() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return !busy; });
  }
  void submit(const char *d, size_t n) {  // (the caller has waited for the writer to be idle)
    std::lock_guard<std::mutex> lk(m);
    data = d; len = n; busy = true;
    cv.notify_all();
  }
  bool finish() {  // everything handed in is written; false if a write failed
    if (!th.joinable()) return true;
    wait_idle();
    { std::lock_guard<std::mutex> lk(m); quit = true; }
    cv.notify_all();
    th.join();
    return !failed;
  }
};

// <out>, the file of matrices, and what every mode that prints one goes through.  A matrix's text is written by a thread of
// its own while the next matrix is fetched, finished and formatted: two buffers ([measured, round 6] 101 matrices of 1000
// individuals, 1.3 GB of text: 8.3 ms a matrix with the write inline).
struct MatrixOut {
  const Pars &p;
  const std::vector<std::string> &labels;
  const uint64_t n_comb;
  FILE *fh;
  Writer writer;
  std::vector<char> text_buf[2];
  uint64_t n_emitted = 0;
  double t_compute = 0, t_write = 0;  // the run's seconds in engine calls and ngd_finish; in formatting and handing to the writer
  std::vector<double> dist;
  std::vector<const char *> label_ptr;
  MatrixOut(const Pars &pars, const std::vector<std::string> &names, uint64_t n_pairs, FILE *f)
      : p(pars), labels(names), n_comb(n_pairs), fh(f), dist(n_pairs) {
    for (auto &l : labels) label_ptr.push_back(l.c_str());
    writer.start(fh);
  }
  // a matrix's print block, ngsDist.cpp:282-287 (join(), gen_func.cpp:479-496); rows formatted in parallel, same bytes
  int64_t format(const double *cells, std::vector<char> &text) const {
    if (text.empty()) text.resize(64 + p.n_ind * (p.n_ind * 16 + 64));
    return format_grown(text, [&](char *buf, size_t cap) { return ngd_format_matrix(cells, p.n_ind, label_ptr.data(), buf, cap, p.n_threads); });
  }
  // one matrix of the output: the reference's progress lines in its order (:218-241, :281), the tail of gen_dist
  // and the print block
  void emit(uint64_t rep, const double *rs, const uint64_t *rc_, const uint64_t *bm, uint64_t n_blocks,
            const double *ready = nullptr /* the matrix's distances, finished already (beside the matrix before it) */,
            int ready_rc = 0, const char *window = nullptr /* --win_size: the window's name; rs, rc_ unused */) {
    if (p.verbose >= 1) {
      if (window) fprintf(stderr, "==> Window %s ...\n", window);
      else if (rep == 0) fprintf(stderr, "==> Analyzing full dataset...\n");
      else fprintf(stderr, "==> Bootstrap replicate # %lu ...\n", rep);
    }
    if (p.verbose >= 2) fprintf(stderr, "> Mapping positions...\n");
    if (rep > 0 && bm && p.verbose >= 5) {
      for (uint64_t b = 0; b < n_blocks; b++)
        for (uint64_t s = 0; s < p.boot_block_size; s++)
          fprintf(stderr, "block: %lu\torig_site: %lu\trand_block:%lu\trand_site: %lu\n", b,
                  b * p.boot_block_size + s, bm[b], bm[b] * p.boot_block_size + s);
    }
    if (p.verbose >= 2) fprintf(stderr, "> Calculating pairwise genetic distances...\n");
    if (p.verbose >= 3 && !window && rs) {  // the per-pair line of ngsDist.cpp:366-367
      uint64_t k = 0;
      for (uint64_t i1 = 0; i1 < p.n_ind; i1++)
        for (uint64_t i2 = i1 + 1; i2 < p.n_ind; i2++, k++)
          fprintf(stderr, "\tDistance of %f from %lu valid sites (%f) between %s (ind %lu) and %s (ind %lu)!\n",
                  rs[k], rc_[k], rs[k] / (double)rc_[k], labels[i1].c_str(), i1, labels[i2].c_str(), i2);
    }
    const double *cells = ready;
    if (ready) {
      if (ready_rc) die("gen_dist", "invalid evolutionary model specified!");
    } else {
      const auto t_f0 = std::chrono::steady_clock::now();
      int rc = ngd_finish(rs, rc_, n_comb, p.tot_sites, p.evol_model, dist.data());
      if (rc) die("gen_dist", "invalid evolutionary model specified!");
      t_compute += since(t_f0);
      cells = dist.data();
    }

    if (p.verbose >= 2) fprintf(stderr, "> Printing distance matrix\n");
    const auto t_w0 = std::chrono::steady_clock::now();
    std::vector<char> &text = text_buf[n_emitted++ & 1];  // (the writer may still be on the other one)
    const int64_t need = format(cells, text);
    if (need < 0) die(kLambda, "cannot format the distance matrix");
    writer.wait_idle();  // the previous matrix is on its way out: matrices are written in order, one at a time
    if (writer.failed) die(kLambda, "cannot write output file!");
    writer.submit(text.data(), (size_t)need);
    t_write += since(t_w0);
  }
};

// --win_boot_rep where every window draws the maps of its own cut-down run (ngd_window_boot_maps; windows of one length
// share them): the table of maps and every window's offset into it.  Returns the table's length.
uint64_t draw_window_maps(const Pars &p, const WindowList &win, uint64_t R, std::vector<uint64_t> &maps, std::vector<uint64_t> &off) {
  off.resize(win.size());
  auto draw = [&](uint64_t *table, uint64_t len) {  // both calls: first the table's length, then the table
    return ngd_window_boot_maps(p.seed, win.lo.data(), win.hi.data(), win.size(), (uint32_t)R, p.boot_block_size, table, len, off.data());
  };
  const int64_t len = draw(nullptr, 0);
  if (len < 0) die(kMain, "cannot draw the windows' block maps!");
  maps.resize((size_t)len + 1);  // (+ 1: never a null table, even where no window holds a block)
  draw(maps.data(), (uint64_t)len);
  return (uint64_t)len;
}

// the maps of a whole-genome job's R replicates, drawn in the order rnd_map_data (ngsDist.cpp:416-437) would draw them
void draw_job_maps(uint32_t rng[3], uint64_t R, uint64_t n_blocks, std::vector<uint64_t> &maps) {
  maps.resize(R * n_blocks + 1);  // (+ 1: never a null table)
  for (uint64_t r = 0; r < R; r++) ngd_boot_block_map(rng, n_blocks, &maps[r * n_blocks]);
}

// The windows go to the engine a group per call, a group being the windows whose results -- bytes_per_window each -- fit
// ~2 GB of host memory: call(w0, n) makes the engine call for windows w0 .. w0 + n - 1, written(w0, n) prints them.
// wait_writer: the last block's text is written before the next group's call.  NGSDIST_WIN_GROUP_MAX in the environment
// (the tests' knob; unset, empty or 0: none) lowers a group to at most that many windows.
template <typename Call, typename Written>
void for_window_groups(const Pars &p, Engine &eng, MatrixOut &out, uint64_t n_win, uint64_t bytes_per_window, bool wait_writer,
                       Call call, Written written) {
  uint64_t per = std::max<uint64_t>(1, std::min<uint64_t>(n_win, (2ull << 30) / bytes_per_window));
  const char *const knob = getenv("NGSDIST_WIN_GROUP_MAX");
  const uint64_t most = knob ? strtoull(knob, nullptr, 10) : 0;
  if (most) per = std::min(per, most);
  for (uint64_t w0 = 0; w0 < n_win; w0 += per) {
    const uint64_t n = std::min(per, n_win - w0);
    const auto t_c0 = std::chrono::steady_clock::now();
    call(w0, n);
    report_fixup(eng.h, p.verbose);
    out.t_compute += since(t_c0);
    written(w0, n);
    if (wait_writer) out.writer.wait_idle();
  }
}

// What run_sets() needs of a mode whose engine calls return SETS: the run's one set -- the full data set and its replicates --
// or one per window.
using EngineCall = std::pair<const char *, int>;  // an entry point's name, as engine_ok prints it, and its return code
struct SetMode {
  const char *no_block;        // the refusal of replicates on fewer sites than one bootstrap block
  uint64_t bytes_per_window;   // of results: what sizes a group of windows
  bool wait_writer = true;     // a group's end waits for <out>'s writer (for_window_groups)
  std::function<void(uint64_t n_sets)> resize;  // the result vectors, for one call
  std::function<EngineCall(const uint64_t *maps, uint64_t n_blocks)> job;  // the whole-genome call
  // the windowed call on n windows: the whole table of maps, the offsets of these windows
  std::function<EngineCall(const uint64_t *lo, const uint64_t *hi, uint64_t n, const uint64_t *maps, uint64_t maps_len,
                           const uint64_t *off)> windows;
  std::function<void(uint64_t w, const char *name, uint64_t k)> write_set;  // set k of the call's results: the run's set w
};

// The driver of --nj, --mds, --mds_align and --boot_stats.  Without windows: the full data set and all its replicates in ONE
// call, their maps drawn in the reference's order.  With windows: a group of them per call (for_window_groups), every window
// with the maps of its own cut-down run (--win_boot_rep; the replicates of a window shorter than one block are 0 / 0), then
// <out>.windows.  window_matrices, group_means, compared_windows, plain_matrices and site_range_matrices keep their own flow --
// one arm, batches of replicates, or one call for all windows: this driver is not for them.
void run_sets(const Pars &p, Engine &eng, const WindowList &win, uint32_t rng[3], MatrixOut &out, const SetMode &mode) {
  const uint64_t R = p.win ? p.win_boot_rep : p.n_boot_rep;
  std::vector<uint64_t> maps(1);
  if (!p.win) {
    const uint64_t n_blocks = R ? (p.n_sites - p.n_sites % p.boot_block_size) / p.boot_block_size : 0;
    if (R && !n_blocks) die(kMain, mode.no_block);
    const auto t_c0 = std::chrono::steady_clock::now();
    draw_job_maps(rng, R, n_blocks, maps);
    mode.resize(1);
    const auto call = mode.job(maps.data(), n_blocks);
    engine_ok(call.first, call.second);
    report_fixup(eng.h, p.verbose);
    out.t_compute += since(t_c0);
    mode.write_set(0, nullptr, 0);
    return;
  }
  std::vector<uint64_t> off(win.size());
  const uint64_t maps_len = R ? draw_window_maps(p, win, R, maps, off) : 0;
  for_window_groups(p, eng, out, win.size(), mode.bytes_per_window, mode.wait_writer,
    [&](uint64_t w0, uint64_t n) {
      mode.resize(n);
      const auto call = mode.windows(&win.lo[w0], &win.hi[w0], n, maps.data(), maps_len, &off[w0]);
      engine_ok(call.first, call.second);
    },
    [&](uint64_t w0, uint64_t n) {
      for (uint64_t k = 0; k < n; k++) mode.write_set(w0 + k, win.name(w0 + k).c_str(), k);
    });
  win.write_file(std::string(p.out) + ".windows", p);
}

// One block of <out>.mds and its kin: "eig" and the K eigenvalues, "total" and tot[0], tot[1] (tot null: no such line), a line
// per row with its label -- label(f, i) writes it and says whether it could -- and the K numbers at(i, k), an empty line; tabs
// between fields, every number as "%.10e".  False: a write failed.
template <typename Label, typename At>
bool write_mds_block(FILE *f, const double *eig, uint32_t K, const double *tot, uint64_t n, Label label, At at) {
  auto numbers = [&](auto value) {  // the K numbers of a line and its end
    bool ok = true;
    for (uint32_t k = 0; k < K; k++) ok = ok && fprintf(f, "\t%.10e", value(k)) > 0;
    return ok && fputc('\n', f) != EOF;
  };
  bool ok = fputs("eig", f) >= 0 && numbers([&](uint32_t k) { return eig[k]; });
  if (tot) ok = ok && fprintf(f, "total\t%.10e\t%.10e\n", tot[0], tot[1]) > 0;
  for (uint64_t i = 0; i < n; i++) ok = ok && label(f, i) && numbers([&](uint32_t k) { return at(i, k); });
  return ok && fputc('\n', f) != EOF;
}

// ---- the site axis in ranges: side by side on the devices, one after the other where they are too small; the matrices of
// the per-range sums added up ----
void site_range_matrices(const Pars &p, const DeviceFit &fit, uint32_t rng[3], uint64_t batch, MatrixOut &out) {
  const uint64_t n_comb = out.n_comb, B = p.boot_block_size;
  const uint64_t n_eff = p.n_boot_rep ? p.n_sites - p.n_sites % B : 0, n_blocks = p.n_boot_rep ? n_eff / B : 0;
  uint64_t unit = 16;  // ranges are whole 16-site groups and whole bootstrap blocks
  if (p.n_boot_rep) { uint64_t a = 16, b = B; while (b) { uint64_t t = a % b; a = b; b = t; } unit = 16 / a * B; }
  // lcm(16, B) can exceed the data set (a large odd block size): then no split into whole units exists, one range
  // is the whole data set, and it only has to fit one device
  const uint64_t whole = (p.n_sites + 15) / 16 * 16;
  if (unit > whole) unit = whole;
  if (fit.budget <= fit.fixed || (fit.budget - fit.fixed) / fit.per_site < unit)
    die(kMain, "not even one range of sites (16 sites / one bootstrap block) fits the device");
  const uint64_t cap = (fit.budget - fit.fixed) / fit.per_site / unit * unit;  // sites one device holds
  const uint64_t n_units = (p.n_sites + unit - 1) / unit;
  const uint64_t G = (uint64_t)p.n_gpus;
  const uint64_t part = std::min(cap, (n_units + G - 1) / G * unit);
  const uint64_t n_parts = (p.n_sites + part - 1) / part;
  if (p.verbose >= 1) {
    if (part < (n_units + G - 1) / G * unit)
      fprintf(stderr, "==> Data set larger than the device budget (%.1f GB): %lu ranges of up to %lu sites\n", fit.budget / 1e9,
              n_parts, part);
    if (G > 1) fprintf(stderr, "==> Site axis split over %lu devices: %lu ranges of up to %lu sites\n", G, n_parts, part);
  }
  // every replicate's block multiplicities, drawn in the reference's order before any data is read
  std::vector<uint32_t> mult((uint64_t)p.n_boot_rep * n_blocks, 0);
  std::vector<uint64_t> maps_kept;
  std::vector<uint64_t> bm(n_blocks);
  for (uint64_t r = 0; r < p.n_boot_rep; r++) {
    ngd_boot_block_map(rng, n_blocks, bm.data());
    for (uint64_t b = 0; b < n_blocks; b++) mult[r * n_blocks + bm[b]]++;
    if (p.verbose >= 5) maps_kept.insert(maps_kept.end(), bm.begin(), bm.end());
  }
  const uint64_t n_mat = p.n_boot_rep + 1;
  // per device: the sums of its ranges, added in ascending range order; devices are added in device order at the
  // end -- a fixed order of additions for given --n_gpus and budget
  std::vector<std::vector<double>> dev_sum(G);
  std::vector<std::vector<uint64_t>> dev_cnt(G);
  std::vector<double> dev_secs(G, 0.0);
  // all matrices of one range: the full data set (ngd_run), then the replicates from their block multiplicities
  auto compute_range = [&](Engine &eng, uint64_t c0, uint64_t c1, uint64_t d) {
    const auto t_c0 = std::chrono::steady_clock::now();
    std::vector<double> &ts = dev_sum[d];
    std::vector<uint64_t> &tc = dev_cnt[d];
    if (ts.empty()) { ts.assign(n_mat * n_comb, 0.0); tc.assign(n_mat * n_comb, 0); }
    std::vector<double> ps(std::min<uint64_t>(batch, n_mat) * n_comb);
    std::vector<uint64_t> pc(ps.size());
    engine_ok("ngd_run", ngd_run(eng.h, nullptr, 0, 0, ps.data(), pc.data()));
    report_fixup(eng.h, p.verbose);
    for (uint64_t k = 0; k < n_comb; k++) { ts[k] += ps[k]; tc[k] += pc[k]; }
    const uint64_t blk_lo = std::min(c0, n_eff) / (B ? B : 1), blk_hi = std::min(c1, n_eff) / (B ? B : 1);
    const uint64_t nb = blk_hi - blk_lo;  // this range's blocks (none in a range of tail sites only)
    std::vector<uint32_t> mpart;
    for (uint64_t r0 = 0; nb && r0 < p.n_boot_rep; r0 += batch) {
      const uint64_t nr = std::min<uint64_t>(batch, p.n_boot_rep - r0);
      mpart.resize(nr * nb);
      for (uint64_t r = 0; r < nr; r++)
        memcpy(&mpart[r * nb], &mult[(r0 + r) * n_blocks + blk_lo], nb * sizeof(uint32_t));
      engine_ok("ngd_run_mult_batch", ngd_run_mult_batch(eng.h, mpart.data(), (uint32_t)nr, nb, B, ps.data(), pc.data()));
      report_fixup(eng.h, p.verbose);
      for (uint64_t k = 0; k < nr * n_comb; k++) {
        ts[(1 + r0) * n_comb + k] += ps[k];
        tc[(1 + r0) * n_comb + k] += pc[k];
      }
    }
    dev_secs[d] += since(t_c0);
  };
  if (p.verbose >= 1) fprintf(stderr, "==> Reading genotype data\n");
  const auto t_l0 = std::chrono::steady_clock::now();
  Loader L(p);
  if (L.seekable() && G > 1) {
    // plain binary file: every device's thread reads its own ranges (nothing is read twice, nothing is replicated)
    // the size check of the whole file, once, with the reference's two messages (read_data.cpp:45-47, :106-109)
    if (L.raw_size < p.n_sites * p.n_ind * 24)
      die("read_geno", "GENO file at premature EOF. Check GENO file and number of sites!");
    L.finish(p.n_sites * p.n_ind * 24 != L.raw_size);
    std::vector<std::thread> th;
    for (uint64_t d = 0; d < G; d++)
      th.emplace_back([&, d]() {
        for (uint64_t k = d; k < n_parts; k += G) {
          const uint64_t c0 = k * part, c1 = std::min(p.n_sites, c0 + part);
          Loader Ld(p, c0);
          Engine eng;
          make_engine(p, eng, c1 - c0, (int)d, true);
          Ld.load(eng, c1 - c0, c1 == p.n_sites);
          Ld.finish(false);
          compute_range(eng, c0, c1, d);
        }
      });
    for (auto &t : th) t.join();
  } else {
    // a stream (gz text, gz binary, stdin) is read front to back by this thread; a range is computed by its device's
    // thread while the next range is read into the next device
    std::vector<std::thread> busy(G);
    for (uint64_t k = 0; k < n_parts; k++) {
      const uint64_t d = k % G, c0 = k * part, c1 = std::min(p.n_sites, c0 + part);
      if (busy[d].joinable()) busy[d].join();  // the device's previous range has left it
      Engine *eng = new Engine();
      make_engine(p, *eng, c1 - c0, (int)d, true);
      L.load(*eng, c1 - c0, c1 == p.n_sites);
      busy[d] = std::thread([&, eng, c0, c1, d]() {
        compute_range(*eng, c0, c1, d);
        delete eng;
      });
    }
    for (auto &t : busy) if (t.joinable()) t.join();
    L.finish();
  }
  const double t_all = since(t_l0);
  double t_dev = 0;
  for (double v : dev_secs) t_dev = std::max(t_dev, v);
  out.t_compute += t_dev;
  if (p.verbose >= 2)
    fprintf(stderr, "> read + prepare + upload + distances of %lu ranges on %lu device(s): %.3f s (%.2f GB of prepared input "
            "in all; slowest device's kernels and copies %.3f s)\n", n_parts, G, t_all, (double)p.n_ind * p.n_sites * 24 / 1e9,
            t_dev);
  std::vector<double> &tot_sum = dev_sum[0];  // (never empty: range 0 is device 0's)
  std::vector<uint64_t> &tot_cnt = dev_cnt[0];
  // devices in ascending order for every cell, cells on --n_threads threads
  parallel_for(p.n_threads, n_mat * n_comb, 1u << 16, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t d = 1; d < G; d++)
      if (!dev_sum[d].empty())
        for (uint64_t k = lo; k < hi; k++) { tot_sum[k] += dev_sum[d][k]; tot_cnt[k] += dev_cnt[d][k]; }
  });
  for (uint64_t rep = 0; rep < n_mat; rep++)
    out.emit(rep, &tot_sum[rep * n_comb], &tot_cnt[rep * n_comb],
             rep && !maps_kept.empty() ? &maps_kept[(rep - 1) * n_blocks] : nullptr, n_blocks);
}

// ---- neighbour-joining trees (--nj): every matrix of every set -- the run's one set, or one per window -- becomes its tree
// on the device (ngd_run_*_nj).  <out> takes matrix 0 of every set (a plain run: the bytes of the run without --nj),
// <out>.nwk one Newick line per matrix, set after set, matrix 0 first, and, with replicates, <out>.support.nwk one line
// per set: matrix 0's tree with the number of replicate trees that share each of its branches ----
void trees(const Pars &p, Engine &eng, const WindowList &win, uint32_t rng[3], MatrixOut &out) {
  const uint64_t R = p.win ? p.win_boot_rep : p.n_boot_rep, n_mat = R + 1, nb = NGD_NJ_NBRANCH(p.n_ind), n_comb = out.n_comb;
  FILE *nf = fopen((std::string(p.out) + ".nwk").c_str(), "w");
  FILE *sf = R ? fopen((std::string(p.out) + ".support.nwk").c_str(), "w") : nullptr;
  if (!nf || (R && !sf)) die(kMain, "cannot open trees output file!");
  std::vector<char> line;
  std::vector<uint32_t> support(p.n_ind > 3 ? p.n_ind - 3 : 1);
  uint64_t n_no_tree = 0;
  auto write_tree = [&](FILE *f, const int32_t *c, const double *l, const uint32_t *sup) {
    const int64_t need = format_grown(line, [&](char *buf, size_t cap) { return ngd_nj_newick(c, l, p.n_ind, out.label_ptr.data(), sup, buf, cap); });
    if (need < 0 || fwrite(line.data(), 1, (size_t)need, f) != (size_t)need) die(kLambda, "cannot write trees output file!");
  };
  std::vector<int32_t> child;
  std::vector<double> len, d0;
  std::vector<uint32_t> status;
  SetMode mode;
  mode.no_block = "neighbour-joining trees (--nj) of bootstrap replicates need at least one bootstrap block of sites!";
  mode.bytes_per_window = n_mat * nb * 12 + n_mat * 4 + n_comb * 8;  // (a window's records and first matrix)
  mode.resize = [&](uint64_t n_sets) {
    child.resize(n_sets * n_mat * nb);
    len.resize(n_sets * n_mat * nb);
    status.resize(n_sets * n_mat);
    d0.resize(n_sets * n_comb);
  };
  mode.job = [&](const uint64_t *maps, uint64_t n_blocks) -> EngineCall {
    return {"ngd_run_job_nj", ngd_run_job_nj(eng.h, maps, (uint32_t)R, n_blocks, p.boot_block_size, p.tot_sites, p.evol_model, child.data(),
                                             len.data(), status.data(), d0.data())};
  };
  // (--win_boot_rep: the replicates of a window shorter than one block have no tree)
  mode.windows = [&](const uint64_t *lo, const uint64_t *hi, uint64_t n, const uint64_t *maps, uint64_t maps_len,
                     const uint64_t *off) -> EngineCall {
    if (!R)
      return {"ngd_run_windows_nj", ngd_run_windows_nj(eng.h, lo, hi, n, p.tot_sites, p.evol_model, child.data(), len.data(), status.data(),
                                                       d0.data())};
    return {"ngd_run_windows_job_var_nj", ngd_run_windows_job_var_nj(eng.h, lo, hi, n, maps, maps_len, off, (uint32_t)R, p.boot_block_size, p.tot_sites,
                                                                     p.evol_model, child.data(), len.data(), status.data(), d0.data())};
  };
  // one set: matrix 0's block through emit() (the progress lines and the writer of any matrix), its trees, its supports
  mode.write_set = [&](uint64_t w, const char *name, uint64_t k) {
    const int32_t *c = &child[k * n_mat * nb];
    const double *l = &len[k * n_mat * nb];
    const uint32_t *st = &status[k * n_mat];
    out.emit(w, nullptr, nullptr, nullptr, 0, &d0[k * n_comb], 0, name);
    for (uint64_t r = 0; r < n_mat; r++) {
      write_tree(nf, c + r * nb, l + r * nb, nullptr);
      n_no_tree += st[r] == 0;
    }
    if (!R) return;
    uint32_t used = 0;
    if (ngd_nj_support(c, st, n_mat, p.n_ind, support.data(), &used)) die(kLambda, "cannot count the trees' support!");
    write_tree(sf, c, l, support.data());
  };
  run_sets(p, eng, win, rng, out, mode);
  if (n_no_tree)
    fprintf(stderr, "WARNING: %lu of the run's matrices have a cell that is not finite and no tree (a line \";\" in %s.nwk)\n",
            (unsigned long)n_no_tree, p.out);
  if (fclose(nf) != 0 || (sf && fclose(sf) != 0)) die(kMain, "cannot write trees output file!");
}

// ---- classical MDS (--mds K): every matrix of every set -- the run's one set, or one per window -- becomes the top K
// eigenpairs of its double-centred form on the device (ngd_run_*_mds).  <out> takes matrix 0 of every set (a plain run: the
// bytes of the run without --mds), <out>.mds one block per matrix, set after set, matrix 0 first: "eig" and the K
// eigenvalues, "total" and the sum of all eigenvalues and of the positive ones, a line per individual with its label and K
// coordinates, an empty line; tabs between fields, every number as "%.10e" ----
void coordinates(const Pars &p, Engine &eng, const WindowList &win, uint32_t rng[3], MatrixOut &out) {
  const uint64_t R = p.win ? p.win_boot_rep : p.n_boot_rep, n_mat = R + 1, n = p.n_ind, n_comb = out.n_comb;
  const uint32_t K = (uint32_t)p.mds_dim;
  FILE *mf = fopen((std::string(p.out) + ".mds").c_str(), "w");
  if (!mf) die(kMain, "cannot open coordinates output file!");
  std::vector<double> xy(n * K);
  uint64_t n_bad = 0;
  std::vector<double> eig, vec, tot, d0;
  std::vector<uint32_t> status;
  SetMode mode;
  mode.no_block = "classical MDS (--mds) of bootstrap replicates needs at least one bootstrap block of sites!";
  mode.bytes_per_window = n_mat * (K * (n + 1) + 2) * 8 + n_mat * 4 + n_comb * 8;  // (a window's outputs and first matrix)
  mode.resize = [&](uint64_t n_sets) {
    eig.resize(n_sets * n_mat * K);
    vec.resize(n_sets * n_mat * K * n);
    tot.resize(n_sets * n_mat * 2);
    status.resize(n_sets * n_mat);
    d0.resize(n_sets * n_comb);
  };
  mode.job = [&](const uint64_t *maps, uint64_t n_blocks) -> EngineCall {
    return {"ngd_run_job_mds", ngd_run_job_mds(eng.h, maps, (uint32_t)R, n_blocks, p.boot_block_size, p.tot_sites, p.evol_model, K, eig.data(),
                                               vec.data(), tot.data(), status.data(), d0.data())};
  };
  // (--win_boot_rep: the replicates of a window shorter than one block have no coordinates)
  mode.windows = [&](const uint64_t *lo, const uint64_t *hi, uint64_t nw, const uint64_t *maps, uint64_t maps_len,
                     const uint64_t *off) -> EngineCall {
    if (!R)
      return {"ngd_run_windows_mds", ngd_run_windows_mds(eng.h, lo, hi, nw, p.tot_sites, p.evol_model, K, eig.data(), vec.data(), tot.data(),
                                                         status.data(), d0.data())};
    return {"ngd_run_windows_job_var_mds", ngd_run_windows_job_var_mds(eng.h, lo, hi, nw, maps, maps_len, off, (uint32_t)R, p.boot_block_size, p.tot_sites,
                                                                       p.evol_model, K, eig.data(), vec.data(), tot.data(), status.data(), d0.data())};
  };
  // one set: matrix 0's block through emit() (the progress lines and the writer of any matrix), then its matrices' blocks
  mode.write_set = [&](uint64_t w, const char *name, uint64_t k) {
    out.emit(w, nullptr, nullptr, nullptr, 0, &d0[k * n_comb], 0, name);
    for (uint64_t m = k * n_mat; m < (k + 1) * n_mat; m++) {
      if (ngd_mds_coords(&eig[m * K], &vec[m * K * n], 1, n, K, xy.data())) die(kLambda, "cannot derive the coordinates!");
      n_bad += status[m] == 0;
      if (!write_mds_block(mf, &eig[m * K], K, &tot[m * 2], n, [&](FILE *f, uint64_t i) { return fputs(out.label_ptr[i], f) >= 0; },
                           [&](uint64_t i, uint32_t d) { return xy[i * K + d]; }))
        die(kLambda, "cannot write coordinates output file!");
    }
  };
  run_sets(p, eng, win, rng, out, mode);
  if (n_bad)
    fprintf(stderr, "WARNING: %lu of the run's matrices have a cell that is not finite and no coordinates (\"nan\" throughout their blocks in %s.mds)\n",
            (unsigned long)n_bad, p.out);
  if (fclose(mf) != 0) die(kMain, "cannot write coordinates output file!");
}

// ---- aligned replicates (--mds K --mds_align): the replicates of every set stay on the device, which rotates their
// coordinates onto matrix 0's and reduces every coordinate and eigenvalue to five statistics (ngd_run_*_mds_align).  <out>
// and <out>.mds take matrix 0 of every set (--mds' blocks); <out>.mds_mean / _sd / _lo / _hi the other statistics in the same
// blocks -- "eig" and the statistic of the K eigenvalues, a line per individual with its label and the statistic of its K
// aligned coordinates, an empty line; no "total" line --; <out>.mds_fit a line per set: the replicates that went in, then
// every replicate's fit ("nan": left out) ----
void aligned_coordinates(const Pars &p, Engine &eng, const WindowList &win, uint32_t rng[3], MatrixOut &out) {
  const uint64_t R = p.win ? p.win_boot_rep : p.n_boot_rep, n_mat = R + 1, n = p.n_ind, n_comb = out.n_comb;
  const uint32_t K = (uint32_t)p.mds_dim;
  const uint64_t n_cells = K * (n + 1);
  static const char *const kSuffix[NGD_BOOT_NSTAT + 1] = {".mds", ".mds_mean", ".mds_sd", ".mds_lo", ".mds_hi", ".mds_fit"};
  FILE *sf[NGD_BOOT_NSTAT + 1];
  for (int k = 0; k <= NGD_BOOT_NSTAT; k++)
    if (!(sf[k] = fopen((std::string(p.out) + kSuffix[k]).c_str(), "w"))) die(kMain, "cannot open coordinates output file!");
  std::vector<double> xy(n * K);
  uint64_t n_bad = 0;
  std::vector<double> eig0, vec0, tot0, stats, fit, d0;
  std::vector<uint32_t> status;
  std::vector<uint64_t> used;
  SetMode mode;
  mode.no_block = "aligned replicates (--mds_align) need at least one bootstrap block of sites!";
  mode.bytes_per_window = ((NGD_BOOT_NSTAT + 1) * n_cells + 3) * 8 + n_mat * 12 + n_comb * 8;  // (a window's outputs and first matrix)
  mode.resize = [&](uint64_t n_sets) {
    eig0.resize(n_sets * K);
    vec0.resize(n_sets * K * n);
    tot0.resize(n_sets * 2);
    status.resize(n_sets * n_mat);
    stats.resize(n_sets * NGD_BOOT_NSTAT * n_cells);
    used.resize(n_sets);
    fit.resize(n_sets * n_mat);
    d0.resize(n_sets * n_comb);
  };
  mode.job = [&](const uint64_t *maps, uint64_t n_blocks) -> EngineCall {
    return {"ngd_run_job_mds_align",
            ngd_run_job_mds_align(eng.h, maps, (uint32_t)R, n_blocks, p.boot_block_size, p.tot_sites, p.evol_model, K, p.mds_ci, eig0.data(),
                                  vec0.data(), tot0.data(), status.data(), stats.data(), used.data(), fit.data(), nullptr, d0.data())};
  };
  // (the replicates of a window shorter than one block are left out: used 0)
  mode.windows = [&](const uint64_t *lo, const uint64_t *hi, uint64_t nw, const uint64_t *maps, uint64_t maps_len,
                     const uint64_t *off) -> EngineCall {
    return {"ngd_run_windows_job_var_mds_align",
            ngd_run_windows_job_var_mds_align(eng.h, lo, hi, nw, maps, maps_len, off, (uint32_t)R, p.boot_block_size, p.tot_sites, p.evol_model, K,
                                              p.mds_ci, eig0.data(), vec0.data(), tot0.data(), status.data(), stats.data(), used.data(),
                                              fit.data(), nullptr, d0.data())};
  };
  // one set: matrix 0's block through emit(), then its blocks and its line of fits
  mode.write_set = [&](uint64_t w, const char *name, uint64_t k) {
    out.emit(w, nullptr, nullptr, nullptr, 0, &d0[k * n_comb], 0, name);
    if (ngd_mds_coords(&eig0[k * K], &vec0[k * K * n], 1, n, K, xy.data())) die(kLambda, "cannot derive the coordinates!");
    for (uint64_t r = 0; r < n_mat; r++) n_bad += status[k * n_mat + r] == 0;
    auto label = [&](FILE *f, uint64_t i) { return fputs(out.label_ptr[i], f) >= 0; };
    // matrix 0's own coordinates [n][K]; of the other statistics the cells [K][n], then their [K] eigenvalues
    bool ok = write_mds_block(sf[0], &eig0[k * K], K, &tot0[k * 2], n, label, [&](uint64_t i, uint32_t d) { return xy[i * K + d]; });
    for (int s = 1; s < NGD_BOOT_NSTAT; s++) {
      const double *cell = &stats[(k * NGD_BOOT_NSTAT + s) * n_cells];
      ok = ok && write_mds_block(sf[s], cell + K * n, K, nullptr, n, label, [&](uint64_t i, uint32_t d) { return cell[d * n + i]; });
    }
    FILE *ff = sf[NGD_BOOT_NSTAT];
    ok = ok && fprintf(ff, "%lu", (unsigned long)used[k]) > 0;
    for (uint64_t r = 1; r < n_mat; r++) {
      const double v = fit[k * n_mat + r];
      ok = ok && (std::isnan(v) ? fputs("\tnan", ff) >= 0 : fprintf(ff, "\t%.10e", v) > 0);
    }
    if (!ok || fputc('\n', ff) == EOF) die(kLambda, "cannot write coordinates output file!");
  };
  run_sets(p, eng, win, rng, out, mode);
  if (n_bad)
    fprintf(stderr, "WARNING: %lu of the run's matrices have a cell that is not finite and no coordinates (they are left out of the summaries in %s.mds_*)\n",
            (unsigned long)n_bad, p.out);
  for (int k = 0; k <= NGD_BOOT_NSTAT; k++)
    if (fclose(sf[k]) != 0) die(kMain, "cannot write coordinates output file!");
}

// ---- bootstrap summaries (--boot_stats): the replicates of every set -- the run's, or a window's -- stay on the device,
// which reduces each cell to five statistics and a count (ngd_run_*_stats).  <out> takes the estimates (matrix 0 of every
// set: the bytes of the run without replicates), <out>.boot_mean / _sd / _lo / _hi the other statistics in the same blocks
// and <out>.boot_used the finite replicates behind them, as integers; with --groups the blocks are G x G ----
void bootstrap_summaries(const Pars &p, Engine &eng, const WindowList &win, const std::vector<int32_t> &group_of,
                         const std::vector<std::string> &group_names, uint32_t rng[3], MatrixOut &out) {
  const bool grp = p.in_groups != nullptr;
  if (grp) engine_ok("ngd_set_groups", ngd_set_groups(eng.h, group_of.data(), (uint32_t)group_names.size()));
  const uint64_t G = group_names.size(), n_cells = grp ? G * (G + 1) / 2 : out.n_comb, n_ind = p.n_ind;
  static const char *const kSuffix[NGD_BOOT_NSTAT + 1] = {"", ".boot_mean", ".boot_sd", ".boot_lo", ".boot_hi", ".boot_used"};
  FILE *sf[NGD_BOOT_NSTAT + 1] = {out.fh};
  for (int k = 1; k <= NGD_BOOT_NSTAT; k++)
    if (!(sf[k] = fopen((std::string(p.out) + kSuffix[k]).c_str(), "w"))) die(kMain, "cannot open bootstrap summaries output file!");
  std::vector<char> text;
  std::string txt, cnt, skip;
  const uint64_t R = p.win ? p.win_boot_rep : p.n_boot_rep;
  std::vector<double> stats;
  std::vector<uint64_t> used;
  SetMode mode;
  mode.no_block = "bootstrap summaries (--boot_stats) need at least one bootstrap block of sites!";
  mode.bytes_per_window = 8 * (NGD_BOOT_NSTAT + 1) * std::max<uint64_t>(1, n_cells);  // (a window's statistics)
  mode.wait_writer = !grp;  // (group pairs are written here, not by the writer thread: nothing to wait for at a group's end)
  mode.resize = [&](uint64_t n_sets) {
    stats.resize(n_sets * NGD_BOOT_NSTAT * n_cells);
    used.resize(n_sets * n_cells);
  };
  mode.job = [&](const uint64_t *maps, uint64_t n_blocks) -> EngineCall {
    return {grp ? "ngd_run_job_groups_stats" : "ngd_run_job_stats",
            (grp ? ngd_run_job_groups_stats : ngd_run_job_stats)(eng.h, maps, (uint32_t)R, n_blocks, p.boot_block_size, p.tot_sites, p.evol_model,
                                                                 p.boot_ci, stats.data(), used.data())};
  };
  // (a window shorter than one block has replicates of 0 / 0: no finite replicate)
  mode.windows = [&](const uint64_t *lo, const uint64_t *hi, uint64_t n, const uint64_t *maps, uint64_t maps_len,
                     const uint64_t *off) -> EngineCall {
    return {grp ? "ngd_run_windows_job_var_groups_stats" : "ngd_run_windows_job_var_stats",
            (grp ? ngd_run_windows_job_var_groups_stats : ngd_run_windows_job_var_stats)(
                eng.h, lo, hi, n, maps, maps_len, off, (uint32_t)R, p.boot_block_size, p.tot_sites, p.evol_model, p.boot_ci, stats.data(), used.data())};
  };
  // one set's blocks: est through emit() (pairs: the progress lines and the writer of any matrix), the rest formatted here
  mode.write_set = [&](uint64_t w, const char *name, uint64_t set) {
    const double *st = stats.data() + set * NGD_BOOT_NSTAT * n_cells;
    const uint64_t *us = used.data() + set * n_cells;
    if (grp) {
      for (int k = 0; k < NGD_BOOT_NSTAT; k++) {
        txt.clear();
        (k ? skip : cnt).clear();
        format_groups(group_names, st + k * n_cells, us, txt, k ? skip : cnt);
        if (fwrite(txt.data(), 1, txt.size(), sf[k]) != txt.size()) die(kLambda, "cannot write output file!");
      }
    } else {
      out.emit(w, nullptr, nullptr, nullptr, 0, st, 0, name);
      for (int k = 1; k < NGD_BOOT_NSTAT; k++) {
        const int64_t need = out.format(st + k * n_cells, text);
        if (need < 0 || fwrite(text.data(), 1, (size_t)need, sf[k]) != (size_t)need) die(kLambda, "cannot write output file!");
      }
      // the counts in a matrix's layout: "\n<n_ind>\n", per individual its label and n_ind cells "\t<m>" (0 on the diagonal)
      cnt = "\n" + std::to_string(n_ind) + "\n";
      for (uint64_t i = 0; i < n_ind; i++) {
        cnt += out.labels[i];
        for (uint64_t j = 0; j < n_ind; j++) {
          const uint64_t a = std::min(i, j), b = std::max(i, j);
          cnt += "\t" + std::to_string(i == j ? 0 : (unsigned long)us[a * n_ind - a * (a + 1) / 2 + (b - a - 1)]);
        }
        cnt += "\n";
      }
    }
    if (fwrite(cnt.data(), 1, cnt.size(), sf[NGD_BOOT_NSTAT]) != cnt.size()) die(kLambda, "cannot write output file!");
  };
  run_sets(p, eng, win, rng, out, mode);
  for (int k = 1; k <= NGD_BOOT_NSTAT; k++)
    if (fclose(sf[k]) != 0) die(kMain, "cannot write bootstrap summaries output file!");
}

// ---- group means (--groups): every matrix of the run -- the full data set and its replicates, or the windows and theirs --
// leaves the engine as its G x G table (ngd_run_*_groups): one block per matrix in <out>, in the order of the run without
// --groups, and the same blocks with the numbers of cells behind the means in <out>.used ----
void group_means(const Pars &p, Engine &eng, const WindowList &win, const std::vector<int32_t> &group_of,
                 const std::vector<std::string> &group_names, uint32_t rng[3], uint64_t batch, MatrixOut &out) {
  engine_ok("ngd_set_groups", ngd_set_groups(eng.h, group_of.data(), (uint32_t)group_names.size()));
  const uint64_t G = group_names.size(), n_gp = G * (G + 1) / 2;
  FILE *uf = fopen((std::string(p.out) + ".used").c_str(), "w");
  if (!uf) die(kMain, "cannot open used output file!");
  std::string txt, cnt;
  auto write_blocks = [&](const double *mean, const uint64_t *used, uint64_t n_mat) {
    const auto t_w0 = std::chrono::steady_clock::now();
    txt.clear();
    cnt.clear();
    for (uint64_t m = 0; m < n_mat; m++) format_groups(group_names, mean + m * n_gp, used + m * n_gp, txt, cnt);
    if (fwrite(txt.data(), 1, txt.size(), out.fh) != txt.size() || fwrite(cnt.data(), 1, cnt.size(), uf) != cnt.size())
      die(kLambda, "cannot write output file!");
    out.t_write += since(t_w0);
  };
  std::vector<double> gmean;
  std::vector<uint64_t> gused, maps;
  const auto t_c0 = std::chrono::steady_clock::now();
  if (p.win) {
    // every window and its replicates in one call.  --win_boot_rep: every window draws the maps of its own cut-down run; a
    // window shorter than one block has replicates of 0 / 0, whose means are nan
    const uint64_t n_win = win.size(), R = p.win_boot_rep, n_mat = R + 1;
    gmean.resize(n_win * n_mat * n_gp);
    gused.resize(n_win * n_mat * n_gp);
    if (R) {
      std::vector<uint64_t> off;
      const uint64_t mlen = draw_window_maps(p, win, R, maps, off);
      engine_ok("ngd_run_windows_job_var_groups",
                ngd_run_windows_job_var_groups(eng.h, win.lo.data(), win.hi.data(), n_win, maps.data(), mlen, off.data(), (uint32_t)R,
                                               p.boot_block_size, p.tot_sites, p.evol_model, gmean.data(), gused.data()));
    } else {
      engine_ok("ngd_run_windows_groups", ngd_run_windows_groups(eng.h, win.lo.data(), win.hi.data(), n_win, p.tot_sites, p.evol_model,
                                                                 gmean.data(), gused.data()));
    }
    report_fixup(eng.h, p.verbose);
    out.t_compute += since(t_c0);
    if (p.verbose >= 1) fprintf(stderr, "==> %lu windows, %lu matrices each\n", (unsigned long)n_win, (unsigned long)n_mat);
    write_blocks(gmean.data(), gused.data(), n_win * n_mat);
  } else {
    // the full data set, then the replicates in batches (their maps drawn in the reference's order); a batch after the
    // first goes through the same call and its leading full-data matrix is dropped
    const uint64_t n_sites_b = p.n_sites - p.n_sites % p.boot_block_size, n_blocks = n_sites_b / p.boot_block_size;
    for (uint64_t rep = 0; rep <= p.n_boot_rep;) {
      const auto t_b0 = std::chrono::steady_clock::now();
      const uint64_t n_here = std::min<uint64_t>(batch - 1, p.n_boot_rep - (rep ? rep - 1 : 0));  // replicates of this call
      gmean.assign((n_here + 1) * n_gp, std::nan(""));
      gused.assign((n_here + 1) * n_gp, 0);
      if (n_here && n_blocks) draw_job_maps(rng, n_here, n_blocks, maps);
      // (fewer sites than one block: the replicates visit no site, ngsDist.cpp:236 -- their means stay nan, used 0)
      const uint32_t n_call = n_blocks ? (uint32_t)n_here : 0;
      if (rep == 0 || n_call) {
        engine_ok("ngd_run_job_groups", ngd_run_job_groups(eng.h, maps.data(), n_call, n_blocks, p.boot_block_size, p.tot_sites, p.evol_model,
                                                           gmean.data(), gused.data()));
        report_fixup(eng.h, p.verbose);
      }
      out.t_compute += since(t_b0);
      if (p.verbose >= 1 && rep == 0) fprintf(stderr, "==> Analyzing full dataset...\n");
      if (p.verbose >= 1 && n_here) fprintf(stderr, "==> Bootstrap replicates # %lu to %lu ...\n", rep ? rep : 1, (rep ? rep : 1) + n_here - 1);
      const uint64_t skip = rep ? 1 : 0;
      write_blocks(gmean.data() + skip * n_gp, gused.data() + skip * n_gp, n_here + 1 - skip);
      rep = (rep ? rep : 1) + n_here;
    }
  }
  if (fclose(uf) != 0) die(kMain, "cannot write used output file!");
  if (p.win) win.write_file(std::string(p.out) + ".windows", p);  // (the windows' own file: as without --groups)
}

// ---- windows along the genome: one matrix per window, in window order, a group of windows per engine call (their
// distances in ~2 GB of host memory), each window's block formatted and written like the full data set's ----
void window_matrices(const Pars &p, Engine &eng, const WindowList &win, MatrixOut &out) {
  const uint64_t n_comb = out.n_comb;
  // --win_boot_rep: R replicates inside every window, its R + 1 blocks printed one after the other -- the file is the
  // concatenation of the cut-down runs' files.  Every cut-down run seeds the generator anew and the windows have one
  // length, so ONE set of block maps, drawn from a fresh state, serves them all (ngsDist.cpp:179-180, :235-238, :416-437)
  const uint64_t R = p.win_boot_rep, n_mat = R + 1;
  const uint64_t wb_blocks = R && !p.win_bp ? p.win_size / p.boot_block_size : 0;
  std::vector<uint64_t> wb_maps, wb_off;
  uint64_t wb_len = 0;
  // --win_bp: the windows differ in length, every one draws the maps of its own cut-down run; a window shorter than one
  // block comes back as sum 0 and count 0, printed as 0 / 0 by the call itself
  if (R && p.win_bp) wb_len = draw_window_maps(p, win, R, wb_maps, wb_off);
  if (R && wb_blocks) {
    uint32_t wrng[3];
    ngd_taus_seed(wrng, p.seed);
    draw_job_maps(wrng, R, wb_blocks, wb_maps);
  }
  // (a window shorter than one block: the reference truncates its replicates to 0 sites and prints 0 / 0, ngsDist.cpp:236)
  std::vector<double> wb_empty;
  if (R && !wb_blocks) {
    const std::vector<double> zs(n_comb, 0.0);
    const std::vector<uint64_t> zc(n_comb, 0);
    wb_empty.resize(n_comb);
    if (ngd_finish(zs.data(), zc.data(), n_comb, p.tot_sites, p.evol_model, wb_empty.data()))
      die("gen_dist", "invalid evolutionary model specified!");
  }
  const bool job = R && (wb_blocks || p.win_bp);
  const uint64_t n_each = job ? n_mat : 1;  // matrices the engine returns per window
  std::vector<double> wd;
  for_window_groups(p, eng, out, win.size(), 8 * n_each * std::max<uint64_t>(1, n_comb), true,
    [&](uint64_t w0, uint64_t n) {
      wd.resize(n * n_each * n_comb);
      const uint64_t *lo = &win.lo[w0], *hi = &win.hi[w0];
      if (job && p.win_bp)
        engine_ok("ngd_run_windows_job_var_dist",
                  ngd_run_windows_job_var_dist(eng.h, lo, hi, n, wb_maps.data(), wb_len, &wb_off[w0], (uint32_t)R, p.boot_block_size,
                                               p.tot_sites, p.evol_model, wd.data()));
      else if (job)
        engine_ok("ngd_run_windows_job_dist", ngd_run_windows_job_dist(eng.h, lo, hi, n, wb_maps.data(), (uint32_t)R, wb_blocks,
                                                                       p.boot_block_size, p.tot_sites, p.evol_model, wd.data()));
      else
        engine_ok("ngd_run_windows_dist", ngd_run_windows_dist(eng.h, lo, hi, n, p.tot_sites, p.evol_model, wd.data()));
    },
    [&](uint64_t w0, uint64_t n) {
      ngd_windows_info wi;
      if (p.verbose >= 2 && ngd_last_windows && ngd_last_windows(eng.h, &wi) == NGD_OK)  // the plan the engine took
        fprintf(stderr, "> windows %lu to %lu: %lu segments in %lu batches of one pass each, %lu windows by a pass of their own (%.2f ms)\n",
                (unsigned long)w0, (unsigned long)(w0 + n - 1), (unsigned long)wi.segments, (unsigned long)wi.batches,
                (unsigned long)wi.windows_by_pass, wi.ms);
      for (uint64_t k = 0; k < n; k++) {
        const std::string name = win.name(w0 + k);
        out.emit(w0 + k, nullptr, nullptr, nullptr, 0, &wd[k * n_each * n_comb], 0, name.c_str());
        for (uint64_t r = 1; r <= R; r++) {
          const std::string rname = name + ", bootstrap replicate # " + std::to_string(r);
          out.emit(w0 + k, nullptr, nullptr, nullptr, 0, job ? &wd[(k * n_mat + r) * n_comb] : wb_empty.data(), 0, rname.c_str());
        }
      }
    });
  win.write_file(std::string(p.out) + ".windows", p);
}

// ---- the comparison of windows (--win_cmp [--win_cmp_mds K]): the windows' matrices stay on the device, which relates every
// window to every other (ngd_run_windows_cmp: all windows in ONE call, their operand is resident there).  <out> and
// <out>.windows are window_matrices'; <out>.win_cor / <out>.win_rms one line per window of W numbers; <out>.win_cmp per window
// its number, mean, sd = sqrt(gram[w][w] / P) and status; <out>.win_mds the classical MDS of the RMS table of the windows that
// were kept (ngd_mds_host), in the block format of <out>.mds with the window number as label; tabs, "%.10e" ----
void compared_windows(const Pars &p, Engine &eng, const WindowList &win, MatrixOut &out) {
  const uint64_t W = win.size(), n_comb = out.n_comb;
  const uint32_t K = (uint32_t)p.win_cmp_dim;
  if (W > ngd_win_cmp_max_vec()) die(kMain, "too many windows for their comparison (--win_cmp)!");
  std::vector<double> mean(W), gram(W * W), cor(W * W), rms(W * W), wd(W * n_comb);
  std::vector<uint32_t> status(W);
  const auto t_c0 = std::chrono::steady_clock::now();
  engine_ok("ngd_run_windows_cmp", ngd_run_windows_cmp(eng.h, win.lo.data(), win.hi.data(), W, p.tot_sites, p.evol_model, mean.data(),
                                                       gram.data(), status.data(), wd.data()));
  report_fixup(eng.h, p.verbose);
  if (ngd_win_cmp_finish(mean.data(), gram.data(), status.data(), W, n_comb, cor.data(), rms.data()))
    die(kMain, "cannot derive the windows' correlations!");
  out.t_compute += since(t_c0);
  for (uint64_t w = 0; w < W; w++) out.emit(w, nullptr, nullptr, nullptr, 0, &wd[w * n_comb], 0, win.name(w).c_str());
  win.write_file(std::string(p.out) + ".windows", p);
  auto open = [&](const char *suffix) {
    FILE *f = fopen((std::string(p.out) + suffix).c_str(), "w");
    if (!f) die(kLambda, "cannot open window comparison output file!");
    return f;
  };
  auto close = [&](FILE *f, bool ok) {
    if (fclose(f) != 0 || !ok) die(kLambda, "cannot write window comparison output file!");
  };
  auto table = [&](const char *suffix, const std::vector<double> &t) {
    FILE *f = open(suffix);
    bool ok = true;
    for (uint64_t a = 0; a < W; a++)
      for (uint64_t b = 0; b < W; b++) ok = ok && fprintf(f, "%.10e%c", t[a * W + b], b + 1 < W ? '\t' : '\n') > 0;
    close(f, ok);
  };
  table(".win_cor", cor);
  table(".win_rms", rms);
  uint64_t n_bad = 0;
  {
    FILE *f = open(".win_cmp");
    bool ok = fputs("window\tmean\tsd\tstatus\n", f) >= 0;
    for (uint64_t w = 0; w < W; w++) {
      n_bad += status[w] == 0;
      ok = ok && fprintf(f, "%lu\t%.10e\t%.10e\t%u\n", (unsigned long)w, mean[w], std::sqrt(gram[w * W + w] / (double)n_comb), status[w]) > 0;
    }
    close(f, ok);
  }
  if (n_bad)
    fprintf(stderr, "WARNING: %lu of the run's windows have a cell that is not finite and are left out of the comparison (\"nan\" throughout their lines in %s.win_*)\n",
            (unsigned long)n_bad, p.out);
  if (!p.win_cmp_mds) return;
  // the RMS table of the windows that were kept, taken as an ordinary distance matrix
  std::vector<uint64_t> kept, row(W);  // (row[w]: where window w stands among them)
  for (uint64_t w = 0; w < W; w++) {
    row[w] = kept.size();
    if (status[w]) kept.push_back(w);
  }
  const uint64_t n = kept.size();
  if (n < 3) die(kMain, "the ordination of the windows (--win_cmp_mds) needs three windows or more that were kept!");
  if (K > n - 1)
    die(kMain, ("the number of dimensions (--win_cmp_mds K) must lie between 1 and min(windows kept - 1, " + std::to_string(ngd_mds_max_dim()) + ")!").c_str());
  std::vector<double> val(n * (n - 1) / 2), eig(K), vec(K * n), tot(2), xy(n * K);
  uint32_t st = 0;
  uint64_t at = 0;
  for (uint64_t a = 0; a < n; a++)
    for (uint64_t b = a + 1; b < n; b++) val[at++] = rms[kept[a] * W + kept[b]];
  if (ngd_mds_host(val.data(), 1, n, K, eig.data(), vec.data(), tot.data(), &st) || ngd_mds_coords(eig.data(), vec.data(), 1, n, K, xy.data()))
    die(kMain, "cannot derive the windows' coordinates!");
  FILE *f = open(".win_mds");
  // (a row per window of the run, "nan" throughout for one that was not kept)
  close(f, write_mds_block(f, eig.data(), K, tot.data(), W, [](FILE *g, uint64_t w) { return fprintf(g, "%lu", (unsigned long)w) > 0; },
                           [&](uint64_t w, uint32_t k) { return status[w] ? xy[row[w] * K + k] : std::nan(""); }));
}

// ---- the plain run: the full data set and its replicates ----
// One batch of matrices: the full data alone (ngd_run), or the full-data matrix plus the first replicates (ngd_run_job,
// which lets the engine share work between them), or replicates only (ngd_run_batch).  True: the batch's matrices stay
// in the engine and come to the host one at a time, as they are printed (ngd_fetch_matrix): the host holds two n_pairs-long
// buffers, not a batch of them ([measured] 1000 individuals, 101 matrices: the 0.8 GB of zero-filled result vectors and
// their page faults cost 1.5 s, three times the engine's whole job).  False: they are in sum, cnt.
bool run_batch(const Pars &p, Engine &eng, uint64_t n_comb, const uint64_t *maps, uint32_t n_rep, bool with_full, uint64_t n_blocks,
               std::vector<double> &sum, std::vector<uint64_t> &cnt) {
  if (!n_rep || n_blocks == 0) {
    // the full data alone (with_full, no replicates); or fewer sites than one bootstrap block: the reference truncates the
    // replicates to 0 sites (ngsDist.cpp:236), visits none and prints 0/0; the full data set is still a plain run
    const uint64_t n_mat = n_rep + (with_full ? 1 : 0);
    sum.assign(n_mat * n_comb, 0.0);
    cnt.assign(n_mat * n_comb, 0);
    if (with_full) {
      engine_ok("ngd_run", ngd_run(eng.h, nullptr, 0, 0, sum.data(), cnt.data()));
      report_fixup(eng.h, p.verbose);
    }
    return false;
  }
  if (with_full) engine_ok("ngd_run_job", ngd_run_job(eng.h, maps, n_rep, n_blocks, p.boot_block_size, nullptr, nullptr));
  else engine_ok("ngd_run_batch", ngd_run_batch(eng.h, maps, n_rep, n_blocks, p.boot_block_size, nullptr, nullptr));
  report_fixup(eng.h, p.verbose);
  return true;
}

// A batch's matrices come out of the engine one at a time -- and matrix r + 1 is fetched and finished (ngd_fetch_matrix,
// ngd_finish) by a thread of its own while matrix r is formatted and handed to the writer: two sets of buffers
struct Pre {
  std::vector<double> sum, dist;
  std::vector<uint64_t> cnt;
  int rc_fetch = 0, rc_finish = 0;
  std::string err;
  std::thread th;
};
// prints the n_in_batch matrices the engine holds, the run's matrices rep, rep + 1, ...; bm_of(r): matrix r's block map
template <typename MapOf>
void emit_fetched(const Pars &p, Engine &eng, MatrixOut &out, uint64_t rep, uint64_t n_in_batch, uint64_t n_blocks, MapOf bm_of) {
  const uint64_t n_comb = out.n_comb;
  Pre pre[2];
  auto start = [&](uint64_t r) {
    Pre &q = pre[r & 1];
    q.sum.resize(n_comb); q.dist.resize(n_comb); q.cnt.resize(n_comb);
    q.th = std::thread([&q, r, &eng, &p, n_comb]() {
      q.rc_fetch = ngd_fetch_matrix(eng.h, (uint32_t)r, q.sum.data(), q.cnt.data());
      if (q.rc_fetch) { q.err = ngd_last_error(); return; }  // (the message is the fetching thread's)
      q.rc_finish = ngd_finish(q.sum.data(), q.cnt.data(), n_comb, p.tot_sites, p.evol_model, q.dist.data());
    });
  };
  start(0);
  for (uint64_t r = 0; r < n_in_batch; r++) {
    Pre &q = pre[r & 1];
    const auto t_g0 = std::chrono::steady_clock::now();
    q.th.join();
    out.t_compute += since(t_g0);
    if (q.rc_fetch) die("ngd_fetch_matrix", (std::string("engine error ") + std::to_string(q.rc_fetch) + ": " + q.err).c_str());
    if (r + 1 < n_in_batch) start(r + 1);
    out.emit(rep + r, q.sum.data(), q.cnt.data(), bm_of(r), n_blocks, q.dist.data(), q.rc_finish);
  }
}

// Matrices go to the engine in batches: the first batch is the full-data matrix plus the first replicates, later ones
// replicates only (run_batch).  The block maps of a batch are drawn up front, in the order rnd_map_data
// (ngsDist.cpp:416-437) would draw them -- nothing else consumes the generator.
void plain_matrices(const Pars &p, Engine &eng, uint32_t rng[3], uint64_t batch, MatrixOut &out) {
  const uint64_t n_comb = out.n_comb;
  std::vector<double> sum;
  std::vector<uint64_t> cnt, block_maps;
  uint64_t n_sites = p.n_sites;
  for (uint64_t rep = 0; rep <= p.n_boot_rep;) {
    const auto t_c0 = std::chrono::steady_clock::now();
    const bool with_full = rep == 0;
    const uint64_t n_in_batch = std::min<uint64_t>(batch, p.n_boot_rep - rep + 1);  // matrices of this batch
    const uint64_t n_boot_here = n_in_batch - (with_full ? 1 : 0);
    uint64_t n_blocks = 0;
    if (n_boot_here) {  // ngsDist.cpp:235-238
      n_sites -= n_sites % p.boot_block_size;
      n_blocks = n_sites / p.boot_block_size;
      draw_job_maps(rng, n_boot_here, n_blocks, block_maps);
    }
    const bool in_engine = run_batch(p, eng, n_comb, block_maps.data(), (uint32_t)n_boot_here, with_full, n_blocks, sum, cnt);
    out.t_compute += since(t_c0);
    auto bm_of = [&](uint64_t r) { return rep + r > 0 ? &block_maps[(r - (with_full ? 1 : 0)) * n_blocks] : nullptr; };
    if (in_engine) emit_fetched(p, eng, out, rep, n_in_batch, n_blocks, bm_of);
    else for (uint64_t r = 0; r < n_in_batch; r++) out.emit(rep + r, &sum[r * n_comb], &cnt[r * n_comb], bm_of(r), n_blocks);
    rep += n_in_batch;
  }
}

}  // namespace

int main(int argc, char **argv) {
  Pars p;
  parse_cmd_args(p, argc, argv);
  const uint64_t n_comb = ngd_n_pairs(p.n_ind);
  if (p.verbose >= 1) fprintf(stderr, "==> Analysis will be run in %lu combinations\n", n_comb);
  input_decisions(p);

  const std::vector<std::string> labels = read_labels(p);
  // --groups: the group of every individual, in input order
  std::vector<int32_t> group_of;
  std::vector<std::string> group_names;
  if (p.in_groups) {
    if (p.verbose >= 1) fprintf(stderr, "==> Reading groups\n");
    read_groups(p.in_groups, group_of, group_names);
    if (group_of.size() != p.n_ind || group_names.empty()) die(__FUNCTION__, "invalid GROUPS file!");
    if (!ngd_set_groups || !ngd_run_job_groups || !ngd_run_windows_groups || !ngd_run_windows_job_var_groups)
      die(__FUNCTION__, "this build of the engine has no group means (--groups)!");
    if (p.verbose >= 1) fprintf(stderr, "==> %lu groups\n", (unsigned long)group_names.size());
  }
  check_summaries_and_trees(p);
  WindowList win;
  if (p.in_pos) read_positions(p, win);
  if (p.win) make_windows(p, win);
  g_phases.mark("args_labels");

  // devices: --n_gpus of them, the site axis split over them
  const int n_dev = ngd_device_count();
  if (n_dev < 1) die(__FUNCTION__, "no HIP device found (this program has no CPU path)");
  if (p.device + (p.same_device ? 1 : p.n_gpus) > n_dev) die(__FUNCTION__, "not enough HIP devices for --device/--n_gpus");
  uint64_t dev_free = 0, dev_total = 0;
  if (ngd_device_memory(p.device, &dev_free, &dev_total)) die_engine("ngd_device_memory", -1);
  g_phases.mark("first_hip_calls");
  const DeviceFit fit = device_fit(p, n_comb, dev_free);
  const struct { bool on; const char *what; } one_gpu[] = {{p.win, "windows (--win_size)"},
                                                           {p.boot_stats, "bootstrap summaries (--boot_stats)"},
                                                           {p.nj, "neighbour-joining trees (--nj)"},
                                                           {p.mds, "classical MDS (--mds)"},
                                                           {p.in_groups != nullptr, "group means (--groups)"}};
  for (auto &m : one_gpu)
    if (m.on && fit.in_parts)
      die(__FUNCTION__, (std::string(m.what) + " need the whole data set on one GPU; it does not fit the device budget!").c_str());

  if (p.verbose >= 2) fprintf(stderr, "==> Setting seed for random number generator\n");
  uint32_t rng[3];
  ngd_taus_seed(rng, p.seed);  // gsl_rng_alloc(gsl_rng_taus) + gsl_rng_set, ngsDist.cpp:179-180

  FILE *out_fh = fopen(p.out, "w");
  if (!out_fh) die(__FUNCTION__, "cannot open output file!");
  MatrixOut out(p, labels, n_comb, out_fh);
  // Matrices per engine call.  --indep_geno: 32 (the engine forms 32 replicates per pass over the per-block partials).
  // EM path: the per-site EM does not depend on the replicate and ONE pass of it serves every matrix of a call (the
  // engine spills the per-(pair, site) terms and contracts them with all the weight vectors: contract_mfma.hip), so the
  // whole job goes in one call where its results (16 B per cell) and block maps fit a few GB of host memory.
  uint64_t batch = 32;
  if (!p.indep_geno && p.n_boot_rep + 1 > batch) {
    const uint64_t by_results = (4ull << 30) / std::max<uint64_t>(1, n_comb * 16);
    const uint64_t blocks = p.boot_block_size ? p.n_sites / p.boot_block_size : 0;
    const uint64_t by_maps = blocks ? (2ull << 30) / (blocks * 8) : ~0ull;
    batch = std::max<uint64_t>(batch, std::min({by_results, by_maps, (uint64_t)p.n_boot_rep + 1}));
  }
  fflush(stdout);

  // exactly one mode writes the run's matrices
  if (fit.in_parts) {
    site_range_matrices(p, fit, rng, batch, out);
  } else {
    Engine eng;  // (the scope of the run's one engine: gone, or left to the exit, before the "destroy" mark)
    make_engine(p, eng, p.n_sites, 0, false);
    g_phases.mark("create");
    if (p.verbose >= 1) fprintf(stderr, "==> Reading genotype data\n");
    const auto t_load0 = std::chrono::steady_clock::now();
    {
      Loader L(p);
      L.load(eng, p.n_sites, true);
      L.finish();
    }
    const double t_load = since(t_load0);
    g_phases.mark("load");
    if (p.verbose >= 2)
      fprintf(stderr, "> read + prepare + upload: %.3f s (%.2f GB of prepared input resident on the device)\n", t_load,
              (double)p.n_ind * p.n_sites * 24 / 1e9);
    if (p.nj) trees(p, eng, win, rng, out);
    else if (p.mds_align) aligned_coordinates(p, eng, win, rng, out);
    else if (p.mds) coordinates(p, eng, win, rng, out);
    else if (p.boot_stats) bootstrap_summaries(p, eng, win, group_of, group_names, rng, out);
    else if (p.in_groups) group_means(p, eng, win, group_of, group_names, rng, batch, out);
    else if (p.win_cmp) compared_windows(p, eng, win, out);
    else if (p.win) window_matrices(p, eng, win, out);
    else plain_matrices(p, eng, rng, batch, out);
    g_phases.mark("matrices");
    eng.leave_to_exit = true;
  }
  g_phases.mark("destroy");
  if (!out.writer.finish()) die(__FUNCTION__, "cannot write output file!");
  g_phases.mark("write_tail");
  fclose(out_fh);
  if (p.verbose >= 2) {
    fprintf(stderr, "> distances: %.3f s for %lu matri%s of %lu pairs; formatting + writing them: %.3f s\n", out.t_compute,
            p.n_boot_rep + 1, p.n_boot_rep ? "ces" : "x", n_comb, out.t_write);
    g_phases.add("of_matrices_distances", out.t_compute);
    g_phases.add("of_matrices_format_write", out.t_write);
    g_phases.print();
  }
  if ((p.em_exact || p.em_exact_boot || p.em_exact_win) && p.verbose >= 1)
    fprintf(stderr, "==> em_exact: %lu (pair, site)s within rounding of the EM's tolerance rechecked, %lu moved to the reference's step\n",
            (unsigned long)g_exact_noted, (unsigned long)g_exact_changed);
  if (p.verbose >= 1) fprintf(stderr, "==> Freeing memory...\n");
  if (p.verbose >= 1) fprintf(stderr, "Done!\n");
  return 0;
}
