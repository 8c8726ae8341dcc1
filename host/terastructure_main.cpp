// terastructure (MI355X host) -- command-line front end over libtsamd.
//
// Keeps the reference's command-line surface and on-disk outputs so that
// data/run.sh works with only the binary path changed:
//   flags                src/main.cc:84-187   (dead flags accepted and ignored)
//   run directory, param.txt, network.dat symlink   src/env.hh:251-311
//   validation sample    src/snpsamplinge.cc:196-224
//   init_gamma           src/snpsamplinge.cc:226-237
//   infer loop, reports  src/snpsamplinge.cc:417-459
//   held-out likelihood, stop rule   src/snpsamplinge.cc:461-544
//   gamma.txt / theta.txt / beta.txt src/snpsamplinge.cc:546-587, :761-798
//   -compute-beta        src/snpsamplinge.cc:74-95, :368-413, :800-862
// The SVI inner loop itself (optimize_lambda + deferred gamma step) runs on the GPU
// behind include/tsamd.h.  There is no CPU path.  `-bfile <prefix>` is accepted as an
// alias of `-file <prefix>.bed`.
#include <errno.h>
#include <math.h>
#include <signal.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <fcntl.h>

#include <algorithm>
#include <limits>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <sstream>
#include <string>
#include <vector>

#include "checkpoint.h"
#include "fast_format.h"
#include "model_writer.h"
#include "tsamd.h"

namespace {

// host/checkpoint.h carries the engine's blob header under its own name (it is built without libtsamd's header)
static_assert(sizeof(ckpt::BlobHeader) == sizeof(tsamd_state_header) && offsetof(ckpt::BlobHeader, part) == offsetof(tsamd_state_header, part) &&
                  offsetof(ckpt::BlobHeader, shard_begin) == offsetof(tsamd_state_header, shard_begin) &&
                  offsetof(ckpt::BlobHeader, alpha) == offsetof(tsamd_state_header, alpha) &&
                  offsetof(ckpt::BlobHeader, payload_bytes) == offsetof(tsamd_state_header, payload_bytes) &&
                  offsetof(ckpt::BlobHeader, checksum) == offsetof(tsamd_state_header, checksum),
              "ckpt::BlobHeader mirrors tsamd_state_header");
static_assert(ckpt::kBlobMagic == TSAMD_STATE_MAGIC && ckpt::kBlobVersion == TSAMD_STATE_VERSION && ckpt::kPartIndiv == TSAMD_STATE_PART_INDIV &&
                  ckpt::kPartLoc == TSAMD_STATE_PART_LOC,
              "blob constants of include/tsamd.h");

// ---- GSL-compatible random numbers (gsl_rng_mt19937 / gsl_rng_uniform_int /
// gsl_ran_gamma; the unit normal uses the polar Box-Muller method) -----
struct Mt19937 {
  uint32_t mt[624];
  int mti;
  explicit Mt19937(unsigned long seed = 0) { set(seed); }
  void set(unsigned long s) {
    if (s == 0) s = 4357;  // gsl mt_set
    mt[0] = (uint32_t)(s & 0xffffffffUL);
    for (int i = 1; i < 624; ++i) mt[i] = (uint32_t)(1812433253UL * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (unsigned long)i);
    mti = 624;
  }
  uint32_t get() {
    if (mti >= 624) {
      for (int kk = 0; kk < 624; ++kk) {
        const uint32_t y = (mt[kk] & 0x80000000U) | (mt[(kk + 1) % 624] & 0x7fffffffU);
        mt[kk] = mt[(kk + 397) % 624] ^ (y >> 1) ^ ((y & 1U) ? 0x9908b0dfU : 0U);
      }
      mti = 0;
    }
    uint32_t k = mt[mti++];
    k ^= (k >> 11);
    k ^= (k << 7) & 0x9d2c5680U;
    k ^= (k << 15) & 0xefc60000U;
    k ^= (k >> 18);
    return k;
  }
  uint32_t uniform_int(uint32_t n) {
    const uint32_t scale = 0xffffffffU / n;
    uint32_t k;
    do k = get() / scale;
    while (k >= n);
    return k;
  }
  double uniform_pos() {
    double x;
    do x = get() / 4294967296.0;
    while (x == 0);
    return x;
  }
  double gaussian() {
    double x, y, r2;
    do {
      x = -1 + 2 * uniform_pos();
      y = -1 + 2 * uniform_pos();
      r2 = x * x + y * y;
    } while (r2 > 1.0 || r2 == 0);
    return y * sqrt(-2.0 * log(r2) / r2);
  }
  double gamma(double a, double b) {  // Marsaglia-Tsang
    if (a < 1) {
      const double u = uniform_pos();
      return gamma(1.0 + a, b) * pow(u, 1.0 / a);
    }
    const double d = a - 1.0 / 3.0, c = (1.0 / 3.0) / sqrt(d);
    double x, v, u;
    while (true) {
      do {
        x = gaussian();
        v = 1.0 + c * x;
      } while (v <= 0);
      v = v * v * v;
      u = uniform_pos();
      if (u < 1 - 0.0331 * x * x * x * x) break;
      if (log(u) < 0.5 * x * x + d * (1 - v + log(v))) break;
    }
    return b * d * v;
  }
};

volatile sig_atomic_t g_terminate = 0;
void term_handler(int) {
  printf("Got termination signal. Saving model state and quitting.\n");
  fflush(stdout);
  g_terminate = 1;
}

struct Options {
  std::string datfname = "network.dat", label, eta_type = "default", idfile, locations_file;
  uint32_t n = 0, k = 0, l = 0, rfreq = 10000, nthreads = 6;
  bool rfreq_set = false, force = false, file_suffix = false, save_beta = false, adagrad = false;
  bool use_test_set = false, compute_beta = false, logl = false, loadcmp = false;
  double seed = 0, stop_threshold = 1e-5;
  int device = 0;
  std::vector<int> devices;  // extension: -devices a,b,...: shard the individuals over these GPUs
  uint32_t max_iter = 0;  // extension: stop after this many iterations (0 = reference behaviour)
  unsigned ingest_threads = 0;  // extension: reader threads of the .bed ingest (0 = up to 8)
  bool ingest_only = false;     // extension: read the genotypes into HBM, write param.txt, stop (ingest measurement)
  bool checkpoint = false;      // extension: every save_model after the initial one also writes <run dir>/checkpoint.bin
  std::string resume;           // extension: start from this checkpoint.bin instead of init_gamma
  std::string project;          // extension: fit this cohort's theta against the lambda of this checkpoint.bin, held fixed
  uint32_t project_iters = 100; // -project: updates per individual, at most
  double project_tol = 1e-5;    // -project: an individual stops when its update changes gamma by less (relative mean change)
  std::string kinship;          // extension: relatedness of the individuals listed in this file, with the final model
  double kinship_min = 0.044194173824159216;  // -kinship-min: pairs below are not listed (2^-4.5: third-degree relatives and closer)
  bool scan = false;            // extension: per-SNP fit and association tests of the final model (scan.txt)
  std::string pheno;            // -scan: one trait value per individual from this file
  uint32_t ld = 0;              // extension: -ld <window>: structure-adjusted LD of nearby locations under the final model, and pruning
  bool ld_set = false, ld_rows_set = false;
  double ld_r2 = 0.2;           // -ld-r2: pruning drops a location whose r^2 with a kept one inside the window exceeds this
  double ld_min = 0.05;         // -ld-min: pairs with a smaller r^2 are not listed in ld.txt
  uint32_t ld_rows = 0;         // -ld-rows: rows of the band the host holds at a time (0: as many as 256 MB hold)
  bool theta_se = false;        // extension: standard errors of the final theta, lambda taken as known (theta_se.txt)
  uint32_t theta_se_rows = 65536;  // -theta-se-rows: individuals per tsamd_theta_info call (what the host holds at a time)
};

struct Timing {
  double ingest = 0, validation_sample = 0, init_gamma = 0, training = 0, report = 0, save_blocking = 0, save_writer = 0, save_wait = 0;
  double ckpt_blocking = 0, ckpt_first = 0, resume = 0;  // of save_blocking: exporting the engine state for checkpoint.bin; reading and importing one
  uint64_t ckpt_bytes = 0;
  uint32_t reports = 0, saves = 0, ckpts = 0;
  double project = 0;  // -project: loading the lambda, the fold-in, foldin.txt
  uint32_t project_iters_run = 0, project_converged = 0;
  double logl = 0;  // -logl: evaluating the training likelihood and writing its files
  double kinship = 0;  // -kinship: tsamd_kinship over all locations and writing its files
  uint32_t kinship_pairs = 0;
  double scan = 0;  // -scan: tsamd_snp_scan over all locations and writing scan.txt
  double ld = 0;    // -ld: tsamd_ld over all locations and writing its files
  uint64_t ld_pairs = 0;
  uint32_t ld_kept = 0;
  double theta_se = 0;  // -theta-se: tsamd_theta_info over all locations, tsamd_theta_se and writing theta_se.txt
  uint32_t theta_se_na = 0;
  uint32_t logls = 0;
};

struct Run {
  Options o;
  Timing tm;
  ModelWriter writer;
  std::string prefix;  // run directory
  FILE *plog = nullptr, *logf = nullptr, *vf = nullptr;
  tsamd_ctx *ctx = nullptr;            // shard 0 (the only one on a single GPU)
  std::vector<tsamd_ctx *> ctxs;       // all shards, rank order
  time_t start_time = time(nullptr);
  uint32_t iter = 0;
  uint32_t saved_iter = 0xffffffffu;  // iteration of the last save_model
  std::map<uint32_t, std::vector<uint32_t>> validation;  // loc -> ascending individuals
  // stop rule state (src/snpsamplinge.cc:26-31)
  double prev_h = -2147483647, max_h = -2147483647;
  uint32_t nh = 0;
  Mt19937 *rng = nullptr;  // the run's generator (its state goes into checkpoint.bin)
  std::vector<uint32_t> kin_ids;  // -kinship: the listed individuals (global ids), read and checked before anything is written
  size_t kin_shard = 0;           // ... and the context whose shard holds them all
  std::vector<double> pheno;      // -pheno: the trait (NaN = not phenotyped), read and checked before anything is written
  std::string bed_path;
  std::vector<std::string> labels;      // -idfile: individual labels, echoed into gammasave.txt
  std::vector<uint8_t> text_payload;   // .012 input: the columns re-packed as PLINK codes, kept for read_column
  uint64_t bytes_per_snp = 0;
  bool columns_on_device = false;       // individual-major input: a column exists only in HBM (read_column downloads it)
  // a resident launch that could not get its workgroups resident lowers the context to one launch per pass; the mode is
  // raised again after `raise_in` further schedules, with a back-off that doubles while the tenant keeps coming back
  uint32_t recoveries_seen = 0, raise_in = 0, raise_backoff = 1;
  bool lowered = false;

  std::string file_str(const std::string &f) const { return prefix + f; }
  uint32_t duration() const { return (uint32_t)(time(nullptr) - start_time); }
  void lerr(const char *fmt, ...) {
    if (!logf) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(logf, fmt, ap);
    va_end(ap);
    fputc('\n', logf);
    fflush(logf);
  }
  void plog_u(const char *k, unsigned long v) { fprintf(plog, "%s: %lu\n", k, v), fflush(plog); }
  void plog_d(const char *k, double v) { fprintf(plog, "%s: %.9f\n", k, v), fflush(plog); }
  void plog_b(const char *k, bool v) { fprintf(plog, "%s: %s\n", k, v ? "True" : "False"), fflush(plog); }
};

[[noreturn]] void die(Run &r, const char *what) {
  fprintf(stderr, "error: %s: %s\n", what, tsamd_last_error(r.ctx));
  r.lerr("error: %s: %s", what, tsamd_last_error(r.ctx));
  r.writer.stop();  // (a snapshot already handed over is written out completely: no half-written gamma.txt)
  exit(-1);
}
#define TS(r, call)               \
  do {                            \
    if ((call) != 0) die(r, #call); \
  } while (0)

// ---- the shards (one context per GPU; a single one unless -devices is given) ----------
// Every operation goes to all shards from this thread, like the reference's main thread
// driving its workers: enqueue on every context, then wait for each.
void shard_span(const Run &r, size_t i, uint32_t &begin, uint32_t &count) {
  tsamd_shard_range(r.o.n, (uint32_t)i, (uint32_t)r.ctxs.size(), &begin, &count);
}

void run_all(Run &r, const uint32_t *locs, uint32_t n, int hol_mode) {
  if (r.lowered && r.ctxs.size() == 1 && --r.raise_in == 0u) {
    // a transient tenant must not cost the rest of a multi-hour run its launch mode: try the resident kernels again
    if (tsamd_set_launch_mode(r.ctx, TSAMD_LAUNCH_PER_SCHEDULE) == 0 || tsamd_set_launch_mode(r.ctx, TSAMD_LAUNCH_PER_SNP) == 0) {
      r.lowered = false;
      r.lerr("launch mode raised again after a replayed schedule (next retry distance %u schedules)", r.raise_backoff);
    } else {
      r.raise_in = r.raise_backoff;
    }
  }
  if (tsamd_run_schedule_all(r.ctxs.data(), (uint32_t)r.ctxs.size(), locs, n, hol_mode) != 0) {
    for (tsamd_ctx *c : r.ctxs)
      if (*tsamd_last_error(c)) r.ctx = c;
    die(r, "tsamd_run_schedule_all");
  }
  for (tsamd_ctx *c : r.ctxs)
    if (tsamd_synchronize(c) != 0) {
      r.ctx = c;
      die(r, "tsamd_synchronize");
    }
  // a resident launch that found compute units of its GPU taken was replayed one launch per pass (include/tsamd.h,
  // tsamd_set_launch_mode): the run goes on, the log says so once per event
  uint32_t now = 0;
  if (tsamd_recoveries(r.ctx, &now) == 0 && now != r.recoveries_seen) {
    r.recoveries_seen = now;
    fprintf(stderr, "%s\n", tsamd_last_error(r.ctx));
    r.lerr("%s", tsamd_last_error(r.ctx));
    r.lowered = true;
    r.raise_in = r.raise_backoff;
    r.raise_backoff = std::min<uint32_t>(r.raise_backoff * 2u, 64u);
  }
}

void set_gamma_all(Run &r, const std::vector<double> &g) {
  for (size_t i = 0; i < r.ctxs.size(); ++i) {
    uint32_t b, c;
    shard_span(r, i, b, c);
    TS(r, tsamd_set_gamma(r.ctxs[i], g.data() + (size_t)b * r.o.k));
  }
}

// ---- pinned host memory for the checkpoint snapshots (-checkpoint) ----------------------
// tsamd_state_export fills a buffer of tsamd_host_alloc by one DMA, without the staging copy a pageable one takes.  Pinning
// hundreds of megabytes costs more than the copy it saves, so a buffer the writer thread is done with comes back here and
// the next snapshot takes it: a run pins as many as are in flight at once (one being filled, one waiting, one being
// written) and no more.  get() is the main thread's, put() the writer thread's.
struct PinnedPool {
  std::mutex mu;
  std::vector<std::pair<void *, size_t>> idle;
  static PinnedPool &the() {
    static PinnedPool p;
    return p;
  }
  static void *get(size_t bytes) {
    PinnedPool &p = the();
    {
      std::lock_guard<std::mutex> lk(p.mu);
      for (size_t i = 0; i < p.idle.size(); ++i)
        if (p.idle[i].second == bytes) {
          void *ptr = p.idle[i].first;
          p.idle.erase(p.idle.begin() + (long)i);
          return ptr;
        }
    }
    void *ptr = nullptr;
    return tsamd_host_alloc(&ptr, bytes) == 0 ? ptr : nullptr;
  }
  static void put(void *ptr, size_t bytes) {
    PinnedPool &p = the();
    std::lock_guard<std::mutex> lk(p.mu);
    p.idle.emplace_back(ptr, bytes);
  }
  static void clear() {  // (after the writer has drained: every buffer is back)
    PinnedPool &p = the();
    std::lock_guard<std::mutex> lk(p.mu);
    for (auto &b : p.idle) tsamd_host_free(b.first);
    p.idle.clear();
  }
};
const ckpt::BufSource kPinned = {PinnedPool::get, PinnedPool::put};

void destroy_all(Run &r) {
  PinnedPool::clear();
  for (tsamd_ctx *c : r.ctxs) tsamd_destroy(c);
  r.ctxs.clear();
  r.ctx = nullptr;
}

void usage() {
  fprintf(stdout,
          "Population inference software for SNP data (MI355X build).\n"
          "terastructure [OPTIONS]\n"
          "\t-help\t\tusage\n"
          "\t-file <name>\t PLINK .bed file (SNP-major; .bim/.fam are found next to it), or a .012 text file\n"
          "\t\t\t (one line per location, one character 0/1/2/- per individual)\n"
          "\t-bfile <prefix>\t same as -file <prefix>.bed\n"
          "\t-n <N>\t\t number of individuals\n"
          "\t-l <L>\t\t number of locations\n"
          "\t-k <K>\t\t number of populations (this build: at most 128; the reference takes any K)\n"
          "\t-label\t\t descriptive tag for the output directory\n"
          "\t-force\t\t overwrite existing output directory\n"
          "\t-rfreq <val>\t checks for convergence and logs output every <val> iterations\n"
          "\t-seed <val>\t random seed\n"
          "\t-compute-beta\t compute allele frequencies given ./gamma.txt\n"
          "\t-logl\t\t with every report, the log-likelihood of the training data: a line in likelihood-analysis.txt\n"
          "\t\t\t (validation.txt's format); at the end logl_snp.txt (loc, count, mean) and logl_indiv.txt\n"
          "\t\t\t (count, mean; theta.txt's order)\n"
          "\t-device <id>\t HIP device ordinal (default 0)\n"
          "\t-devices <a,b,..>\t shard the individuals over these HIP devices (one shard each)\n"
          "\t-ingest-threads <T>\t reader threads of the .bed ingest (default: up to 8)\n"
          "\t-ingest-only\t read the genotypes into HBM, report the rate, write param.txt and stop\n"
          "\t-checkpoint\t with every gamma.txt / theta.txt after the initial one, also write <run dir>/checkpoint.bin:\n"
          "\t\t\t the full engine and sampler state of that iteration\n"
          "\t-resume <file>\t continue the run that wrote this checkpoint.bin (same -n -l -k -seed -rfreq and data; any\n"
          "\t\t\t -devices); with the same device count the continuation is bit for bit the uninterrupted\n"
          "\t\t\t run's.  Not together with -compute-beta\n"
          "\t-project <file>\t fit the theta of the individuals in -file against the lambda of this checkpoint.bin, held fixed:\n"
          "\t\t\t -n is THIS cohort's size, -l and -k must be the file's.  Writes theta.txt / gamma.txt and foldin.txt\n"
          "\t\t\t (individual, updates, last change).  Not together with -resume or -compute-beta\n"
          "\t-project-iters <I>\t -project: at most this many updates per individual (default 100)\n"
          "\t-project-tol <t>\t -project: an individual stops once an update changes its gamma by less than this\n"
          "\t\t\t (mean |change| / mean gamma; default 1e-5; 0: always -project-iters updates)\n"
          "\t-kinship <file>\t with the final model (a plain run, -resume or -project): admixture-adjusted relatedness (REAP)\n"
          "\t\t\t of the individuals listed in <file>, one 0-based index per line (at most 32768, all on one\n"
          "\t\t\t device's shard), over all locations.  Writes kinship.txt (i, j, kinship, sum of the pair's\n"
          "\t\t\t sqrt(q (1 - q)) products; pairs i < j at or above -kinship-min) and inbreeding.txt (i, 2 kin_ii - 1)\n"
          "\t-kinship-min <phi>\t -kinship: lowest kinship coefficient listed (default 0.0442 = 2^-4.5: third-degree\n"
          "\t\t\t relatives and closer; a negative value lists every pair)\n"
          "\t-scan\t\t with the final model (a plain run, -resume or -project): per-SNP tests adjusted for structure.\n"
          "\t\t\t Writes scan.txt: loc, n, O0, O1, O2 (genotype counts), E0, E1, E2 (expected under Binomial(2, q)),\n"
          "\t\t\t z_het, p_het (heterozygote count against the model), z_freq, p_freq (allele count against it)\n"
          "\t-pheno <file>\t -scan: one trait value per line (theta.txt's order, exactly -n lines; NA or nan = not\n"
          "\t\t\t phenotyped); scan.txt gains n_t, z_trait, p_trait: the score test of the trait against the\n"
          "\t\t\t genotype residual y - 2q\n"
          "\t-ld <window>\t with the final model (a plain run, -resume or -project): LD of every pair of locations at most\n"
          "\t\t\t <window> (1 to 1024) positions apart, adjusted for structure: the correlation r of the genotype\n"
          "\t\t\t residuals (y - 2q) / sqrt(2q (1 - q)).  Writes ld.txt (i, j, r, r2, n, p; pairs at or above -ld-min)\n"
          "\t\t\t and an LD pruning, prune.in / prune.out: 0-based location indices in -locations-file's format\n"
          "\t-ld-r2 <max>\t -ld: in ascending order a location is pruned when its r2 with a kept location inside the\n"
          "\t\t\t window exceeds this (default 0.2)\n"
          "\t-ld-min <r2>\t -ld: lowest r2 listed in ld.txt (default 0.05; 0 lists every pair of the band)\n"
          "\t-ld-rows <rows>\t -ld: locations whose rows of the band the host holds at a time (default: as many as 256 MB\n"
          "\t\t\t of host memory hold, at least 4096); the files do not depend on it beyond the rounding of r\n"
          "\t-theta-se\t with the final model (a plain run, -resume or -project): standard errors of theta from the observed\n"
          "\t\t\t information over all locations, lambda taken as known.  Writes theta_se.txt: one line per\n"
          "\t\t\t individual in theta.txt's order, K values; NA where an individual's theta is not identified\n"
          "\t-theta-se-rows <n>\t -theta-se: individuals per call, whose K (K + 1) / 2 doubles each the host holds (default 65536)\n");
  fflush(stdout);
}

int count_lines(const std::string &path) {
  FILE *f = fopen(path.c_str(), "r");
  if (!f) return -1;
  int n = 0;
  char buf[20480];
  while (fgets(buf, sizeof buf, f) != nullptr) n++;
  fclose(f);
  return n;
}

// Env::Env directory naming + param.txt (src/env.hh:251-311)
void setup_run_dir(Run &r) {
  const Options &o = r.o;
  std::ostringstream sa;
  sa << "n" << o.n << "-" << "k" << o.k << "-" << "l" << o.l;
  if (o.label != "")
    sa << "-" << o.label;
  else if (o.datfname.length() > 3) {
    std::string q = o.datfname.substr(0, 2);
    if (q == "..") q = "xx";
    sa << "-" << q;
  }
  if (o.seed != 0) sa << "-" << "seed" << o.seed;
  r.prefix = sa.str();
  fprintf(stdout, "+ Creating directory %s\n", r.prefix.c_str());
  struct stat st;
  if (stat(r.prefix.c_str(), &st) != 0) {
    if (errno != ENOENT || mkdir(r.prefix.c_str(), S_IRWXU | S_IRWXG | S_IROTH | S_IXOTH) != 0) {
      fprintf(stderr, "Warning: could not create dir %s\n", r.prefix.c_str());
      exit(-1);
    }
  } else if (!o.force) {
    fprintf(stderr, "Error: dir %s already exists\n", r.prefix.c_str());
    exit(-1);
  }
  r.logf = fopen(r.file_str("/infer.log").c_str(), "w");
  r.plog = fopen(r.file_str("/param.txt").c_str(), "w");
  if (!r.plog || !r.logf) {
    printf("cannot open param file:%s\n", strerror(errno));
    exit(-1);
  }
  const uint32_t blocks = o.n > 10000 ? 100 : 10;
  r.plog_u("n", o.n);
  r.plog_u("k", o.k);
  r.plog_u("t", 2);
  r.plog_u("l", o.l);
  r.plog_u("nthreads", o.nthreads);
  r.plog_d("tau0", 1);
  r.plog_d("nodetau0", 1);
  r.plog_d("kappa", 0.5);
  r.plog_d("nodekappa", 0.5);
  r.plog_d("alpha", 1.0 / o.k);
  r.plog_d("heldout_indiv_ratio", 0.001);
  r.plog_d("validation_ratio", 0.005);
  r.plog_u("online_iterations", 10);
  r.plog_d("GSL seed", o.seed);
  r.plog_b("file suffix", o.file_suffix);
  r.plog_b("save beta", o.save_beta);
  r.plog_b("adagrad", o.adagrad);
  r.plog_u("indiv sample size", o.n / blocks);
  r.plog_u("blocks", blocks);
  r.plog_b("compute_beta", o.compute_beta);
  r.plog_d("stop_threshold", o.stop_threshold);
  r.plog_b("checkpoint", o.checkpoint);
  fprintf(r.plog, "resume: %s\n", o.resume.empty() ? "False" : o.resume.c_str()), fflush(r.plog);
  if (!o.project.empty()) {  // (a line of its own only in a -project run: param.txt of every other run is unchanged)
    fprintf(r.plog, "project: %s\n", o.project.c_str());
    r.plog_u("project_iters", o.project_iters);
    fprintf(r.plog, "project_tol: %.9g\n", o.project_tol), fflush(r.plog);
  }
  const std::string nd = r.file_str("/network.dat");
  unlink(nd.c_str());
  if (symlink(o.datfname.c_str(), nd.c_str()) < 0) fprintf(stderr, "warning: cannot symlink %s\n", nd.c_str());
  fprintf(stderr, "+ done initializing env\n");
}

// SNP::read_bed (src/snp.cc:95-253): line counts must match -l / -n, magic 6c 1b 01,
// then the SNP-major payload goes to HBM as is.
void read_bed(Run &r) {
  const Options &o = r.o;
  const std::string prefix = o.datfname.substr(0, o.datfname.length() - 4);
  const int l = count_lines(prefix + ".bim");
  if (l < 0) {
    fprintf(stderr, "cannot open file %s.bim:%s\n", prefix.c_str(), strerror(errno));
    exit(-1);
  }
  printf("+ bim file tells us %d SNPs\n", l);
  if ((uint32_t)l != o.l) {
    fprintf(stderr, "-l input doesn't match SNPs in bim file\n");
    exit(-1);
  }
  const int n = count_lines(prefix + ".fam");
  if (n < 0) {
    fprintf(stderr, "cannot open file %s.fam:%s\n", prefix.c_str(), strerror(errno));
    exit(-1);
  }
  printf("+ fam file tells us %d individuals\n", n);
  if ((uint32_t)n != o.n) {
    fprintf(stderr, "-n input doesn't match individuals in fam file\n");
    exit(-1);
  }
  r.bed_path = prefix + ".bed";
  r.bytes_per_snp = ((uint64_t)o.n + 3) / 4;
  FILE *f = fopen(r.bed_path.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "cannot open file %s:%s\n", r.bed_path.c_str(), strerror(errno));
    exit(-1);
  }
  unsigned char magic[3];
  if (fread(magic, 1, 3, f) != 3 || magic[0] != 108 || magic[1] != 27) {
    fprintf(stderr, "%s magic number incorrect\n", r.bed_path.c_str());
    exit(-1);
  }
  if (magic[2] == 0) {
    // PLINK individual-major layout: refused by the reference (src/snp.cc:176-178); here the rows are
    // transposed on the device into the SNP-major columns the engine keeps (tsamd_upload_bed_indiv_major)
    printf("+ individual-major .bed: transposing on the device\n");
    const uint64_t bpi = ((uint64_t)o.l + 3) / 4;
    const uint32_t per = (uint32_t)std::max<uint64_t>(16, std::min<uint64_t>(o.n, ((uint64_t)256 << 20) / bpi / 16 * 16));
    std::vector<uint8_t> rows((size_t)per * bpi);
    for (uint32_t i0 = 0; i0 < o.n; i0 += per) {
      const uint32_t ni = std::min(per, o.n - i0);
      if (fread(rows.data(), bpi, ni, f) != ni) {
        fprintf(stderr, "%s is truncated: fewer than %u individuals\n", r.bed_path.c_str(), o.n);
        exit(-1);
      }
      for (tsamd_ctx *c : r.ctxs) TS(r, tsamd_upload_bed_indiv_major(c, rows.data(), bpi, i0, ni));
      printf("\r%d individuals read", i0 + ni);
      fflush(stdout);
    }
    fclose(f);
    r.columns_on_device = true;
    uint64_t cnt[4] = {0, 0, 0, 0};
    for (tsamd_ctx *c : r.ctxs) {
      uint64_t part[4];
      TS(r, tsamd_genotype_counts(c, 0, o.l, part));
      for (int q = 0; q < 4; ++q) cnt[q] += part[q];
    }
    r.plog_u("missing snps", cnt[1]);
    r.plog_u("0s snps", cnt[3]);
    r.plog_u("1s snps", cnt[2]);
    r.plog_u("2s snps", cnt[0]);
    return;
  } else if (magic[2] != 1) {
    fprintf(stderr, "mode problem in %s\n", r.bed_path.c_str());
    exit(-1);
  }
  fclose(f);
  // Streaming ingest: reader threads pread() a batch of columns into one of two pinned buffers
  // while the previous batch's strided DMA into HBM is in flight (tsamd_upload_bed_async, every
  // shard from the same buffer).  The genotype tallies of param.txt are taken on the device
  // afterwards (tsamd_genotype_counts), not one 2-bit code at a time on the host.
  const int fd = open(r.bed_path.c_str(), O_RDONLY);
  if (fd < 0) {
    fprintf(stderr, "cannot open file %s:%s\n", r.bed_path.c_str(), strerror(errno));
    exit(-1);
  }
  struct stat st;
  if (fstat(fd, &st) != 0 || (uint64_t)st.st_size < 3 + (uint64_t)o.l * r.bytes_per_snp) {
    fprintf(stderr, "%s is truncated: %llu of %llu locations\n", r.bed_path.c_str(),
            (unsigned long long)((st.st_size > 3 ? (uint64_t)st.st_size - 3 : 0) / r.bytes_per_snp), (unsigned long long)o.l);
    exit(-1);
  }
  const size_t batch = std::max<size_t>(1, std::min<size_t>((size_t)(256u << 20) / r.bytes_per_snp, o.l));
  uint8_t *buf[2] = {nullptr, nullptr};
  for (auto &b : buf) {
    void *ptr = nullptr;
    if (tsamd_host_alloc(&ptr, batch * r.bytes_per_snp) != 0) {
      fprintf(stderr, "error: %s\n", tsamd_last_error(nullptr));
      exit(-1);
    }
    b = (uint8_t *)ptr;
  }
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const unsigned nread = std::max(1u, std::min({o.ingest_threads ? o.ingest_threads : 8u, hw, (unsigned)batch}));
  auto read_batch = [&](uint8_t *dst, uint32_t loc0, size_t cols) {  // columns [loc0, loc0 + cols) -> dst
    std::vector<std::thread> th;
    std::vector<int> bad(nread, 0);
    for (unsigned t = 0; t < nread; ++t)
      th.emplace_back([&, t]() {
        const size_t c0 = cols * t / nread, c1 = cols * (t + 1) / nread;
        size_t off = c0 * r.bytes_per_snp;
        const size_t end = c1 * r.bytes_per_snp;
        while (off < end) {
          const ssize_t got = pread(fd, dst + off, std::min<size_t>(end - off, (size_t)64 << 20),
                                    3 + (off_t)loc0 * (off_t)r.bytes_per_snp + (off_t)off);
          if (got <= 0) {
            bad[t] = 1;
            return;
          }
          off += (size_t)got;
        }
      });
    for (auto &x : th) x.join();
    for (int b : bad)
      if (b) {
        fprintf(stderr, "cannot read %s\n", r.bed_path.c_str());
        exit(-1);
      }
  };
  const auto t_ing = std::chrono::steady_clock::now();
  uint32_t loc = 0;
  int cur = 0;
  size_t cols = std::min<size_t>(batch, o.l);
  read_batch(buf[cur], 0, cols);
  while (loc < o.l) {
    for (tsamd_ctx *c : r.ctxs) TS(r, tsamd_upload_bed_async(c, buf[cur], r.bytes_per_snp, loc, (uint32_t)cols));
    const uint32_t next = loc + (uint32_t)cols;
    const size_t ncols = std::min<size_t>(batch, o.l - next);
    if (ncols) read_batch(buf[cur ^ 1], next, ncols);        // overlaps the DMA of buf[cur]
    for (tsamd_ctx *c : r.ctxs) TS(r, tsamd_synchronize(c));  // buf[cur] is free again
    loc = next;
    cols = ncols;
    cur ^= 1;
    printf("\r%d locations read", loc);
    fflush(stdout);
  }
  const double ing_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_ing).count();
  close(fd);
  for (auto &b : buf) tsamd_host_free(b);
  printf("\n+ ingest: %.2f GB in %.2f s (%.1f GB/s, %u reader threads)\n", (double)o.l * r.bytes_per_snp / 1e9, ing_s,
         (double)o.l * r.bytes_per_snp / 1e9 / ing_s, nread);
  // tallies over every shard (tail bits of a column's last byte and padding excluded by the kernel)
  uint64_t cnt[4] = {0, 0, 0, 0};
  for (tsamd_ctx *c : r.ctxs) {
    uint64_t part[4];
    TS(r, tsamd_genotype_counts(c, 0, o.l, part));
    for (int q = 0; q < 4; ++q) cnt[q] += part[q];
  }
  r.plog_u("missing snps", cnt[1]);
  r.plog_u("0s snps", cnt[3]);  // labels swapped like the reference (src/snp.cc:207-216, :245-247)
  r.plog_u("1s snps", cnt[2]);
  r.plog_u("2s snps", cnt[0]);
}

// SNP::read, text branch (src/snp.cc:16-92): one line per location, one character per
// individual: '0' '1' '2' = copies of the counted allele, '-' = missing.  Each line is re-packed
// into the PLINK 2-bit codes the engine stores (0 -> 00, 1 -> 10, 2 -> 11, missing -> 01); the
// format is for small data, so the packed columns stay in host memory for the held-out
// sampling.  (The reference reads into a 20 KB line buffer; any line length works here.)
void read_012(Run &r) {
  const Options &o = r.o;
  printf("+ .012 detected");
  fprintf(stdout, "+ reading (%d,%d) snps from %s\n", o.n, o.l, o.datfname.c_str());
  fflush(stdout);
  FILE *f = fopen(o.datfname.c_str(), "r");
  if (!f) {
    r.lerr("cannot open file %s:%s", o.datfname.c_str(), strerror(errno));
    fprintf(stderr, "cannot open file %s:%s\n", o.datfname.c_str(), strerror(errno));
    exit(-1);
  }
  r.bytes_per_snp = ((uint64_t)o.n + 3) / 4;
  r.text_payload.assign((size_t)o.l * r.bytes_per_snp, 0);
  uint64_t missing = 0, a[3] = {0, 0, 0};
  static const uint8_t code_of_y[3] = {0u, 2u, 3u};
  char *line = nullptr;
  size_t cap = 0;
  uint32_t loc = 0;
  while (loc < o.l) {
    ssize_t len = getline(&line, &cap, f);
    if (len < 0) break;
    while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r' || line[len - 1] == ' ')) --len;
    if (len == 0) continue;
    if ((size_t)len < o.n) {
      printf("Error: unexpected lines in file\n");
      exit(-1);
    }
    uint8_t *col = r.text_payload.data() + (size_t)loc * r.bytes_per_snp;
    for (uint32_t i = 0; i < o.n; ++i) {
      uint8_t code;
      if (line[i] == '-') {
        missing++;
        code = 1u;
      } else if (line[i] >= '0' && line[i] <= '2') {
        a[line[i] - '0']++;
        code = code_of_y[line[i] - '0'];
      } else {
        fprintf(stderr, "%s: unexpected character '%c' at location %u\n", o.datfname.c_str(), line[i], loc);
        exit(-1);
      }
      col[i >> 2] |= (uint8_t)(code << (2 * (i & 3)));
    }
    loc++;
    if (loc % 10000 == 0) {
      printf("\r%d locations read", loc);
      fflush(stdout);
    }
  }
  free(line);
  fclose(f);
  if (loc != o.l) {
    fprintf(stderr, "%s is truncated: %u of %u locations\n", o.datfname.c_str(), loc, o.l);
    exit(-1);
  }
  const uint32_t batch = (uint32_t)std::max<size_t>(1, (size_t)(64u << 20) / r.bytes_per_snp);
  for (uint32_t l0 = 0; l0 < o.l; l0 += batch)
    for (tsamd_ctx *c : r.ctxs)
      TS(r, tsamd_upload_bed(c, r.text_payload.data() + (size_t)l0 * r.bytes_per_snp, r.bytes_per_snp, l0,
                             std::min(batch, o.l - l0)));
  r.plog_u("missing snps", missing);
  r.plog_u("0s snps", a[0]);
  r.plog_u("1s snps", a[1]);
  r.plog_u("2s snps", a[2]);
}

std::vector<uint8_t> read_column(Run &r, uint32_t loc) {
  if (r.columns_on_device) {  // shard after shard (shards start on multiples of 4 individuals: whole bytes)
    std::vector<uint8_t> col(r.bytes_per_snp);
    for (size_t i = 0; i < r.ctxs.size(); ++i) {
      uint32_t b, c;
      shard_span(r, i, b, c);
      TS(r, tsamd_download_bed(r.ctxs[i], loc, col.data() + b / 4, ((uint64_t)c + 3) / 4));
    }
    return col;
  }
  if (!r.text_payload.empty())
    return std::vector<uint8_t>(r.text_payload.begin() + (size_t)loc * r.bytes_per_snp,
                                r.text_payload.begin() + (size_t)(loc + 1) * r.bytes_per_snp);
  std::vector<uint8_t> col(r.bytes_per_snp);
  FILE *f = fopen(r.bed_path.c_str(), "rb");
  if (!f || fseeko(f, 3 + (off_t)loc * (off_t)r.bytes_per_snp, SEEK_SET) != 0 ||
      fread(col.data(), 1, col.size(), f) != col.size()) {
    fprintf(stderr, "cannot read location %u of %s\n", loc, r.bed_path.c_str());
    exit(-1);
  }
  fclose(f);
  return col;
}

// set_validation_sample (src/snpsamplinge.cc:196-224): kv_ok = not held out yet, not missing
void set_validation_sample(Run &r, Mt19937 &rng) {
  const uint32_t n = r.o.n, l = r.o.l;
  const uint32_t per_loc_h = n < 2000 ? (n / 10) : (n / 100);
  const double validation_ratio = 0.005;
  const uint32_t nlocs = (uint32_t)(l * validation_ratio);
  std::map<uint32_t, bool> lm;
  do {
    const uint32_t loc = rng.uniform_int(l);
    if (lm.find(loc) != lm.end()) continue;
    lm[loc] = true;
    const std::vector<uint8_t> col = read_column(r, loc);
    std::vector<bool> held(n, false);
    std::vector<uint32_t> &v = r.validation[loc];
    uint32_t c = 0;
    while (c < per_loc_h) {
      const uint32_t indiv = rng.uniform_int(n);
      const uint32_t code = (col[indiv >> 2] >> (2 * (indiv & 3))) & 3;
      if (!held[indiv] && code != 1) {
        held[indiv] = true;
        v.push_back(indiv);
        c++;
      }
    }
    std::sort(v.begin(), v.end());
    if (v.empty())
      r.validation.erase(loc);
    else
      for (tsamd_ctx *c : r.ctxs) TS(r, tsamd_set_heldout(c, loc, v.data(), (uint32_t)v.size()));
  } while (lm.size() < nlocs);
  r.plog_u("validation snps per location", per_loc_h);
  r.plog_u("validation locations", nlocs);
  r.plog_u("total validation snps", (unsigned long)per_loc_h * nlocs);
  size_t total = 0;
  for (auto &kv : r.validation) total += kv.second.size();
  r.plog_u("(VAL1) total validation snps (check)", total);
  r.plog_d("test ratio", 0.005);
  r.plog_d("validation ratio", 0.005);
}

std::string add_iter_suffix(const Run &r, const char *c) {
  std::ostringstream sa;
  if (r.o.file_suffix)
    sa << c << "_" << r.iter << ".txt";
  else
    sa << c << ".txt";
  return r.file_str(sa.str());
}

// save_gamma (src/snpsamplinge.cc:546-576)
// The main thread snapshots gamma / theta; the writer thread formats and writes them (ModelWriter above) while the next
// schedules run.  The file names are fixed here (-file-suffix: the iteration of THIS save).
void save_model(Run &r, bool with_checkpoint = true) {
  Stopwatch sw;
  const size_t n = r.o.n, k = r.o.k;
  std::unique_ptr<SaveJob> job(new SaveJob);
  job->n = n;
  job->k = k;
  job->g.resize(n * k);
  job->t.resize(n * k);
  job->gamma_path = add_iter_suffix(r, "/gamma");
  job->theta_path = add_iter_suffix(r, "/theta");
  for (size_t i = 0; i < r.ctxs.size(); ++i) {
    uint32_t b, c;
    shard_span(r, i, b, c);
    TS(r, tsamd_get_gamma(r.ctxs[i], job->g.data() + (size_t)b * k));
    TS(r, tsamd_get_theta(r.ctxs[i], job->t.data() + (size_t)b * k));
  }
  if (r.o.checkpoint && with_checkpoint) {
    // the whole engine state of this iteration, next to gamma.txt: the location part from context 0 (identical on every
    // shard), every shard's own part, the sampler and the stop rule.  Exported here, written by the writer thread.
    Stopwatch cw;
    job->ckpt_path = r.file_str("/checkpoint.bin");
    ckpt::FileHeader &fh = job->ckpt_head;
    fh.n = r.o.n, fh.l = r.o.l, fh.k = r.o.k, fh.rfreq = r.o.rfreq, fh.nparts = (uint32_t)r.ctxs.size();
    fh.seed = r.o.seed, fh.stop_threshold = r.o.stop_threshold;
    ckpt::HostState &hs = job->ckpt_host;
    hs.iter = r.iter, hs.nh = r.nh, hs.prev_h = r.prev_h, hs.max_h = r.max_h;
    memcpy(hs.mt, r.rng->mt, sizeof hs.mt);
    hs.mti = r.rng->mti;
    job->ckpt_indiv.resize(r.ctxs.size());
    for (size_t i = 0; i < r.ctxs.size(); ++i) {
      uint64_t ib = 0, lb = 0;
      r.ctx = r.ctxs[i];
      TS(r, tsamd_state_sizes(r.ctxs[i], &ib, &lb));
      if (!job->ckpt_indiv[i].alloc(ib, &kPinned) || (i == 0 && !job->ckpt_loc.alloc(lb, &kPinned))) {
        r.lerr("checkpoint: %s\n", tsamd_last_error(nullptr));
        fprintf(stderr, "error: checkpoint: %s\n", tsamd_last_error(nullptr));
        exit(-1);
      }
      TS(r, tsamd_state_export(r.ctxs[i], job->ckpt_indiv[i].data(), ib, i == 0 ? job->ckpt_loc.data() : nullptr, i == 0 ? lb : 0));
      r.tm.ckpt_bytes += ib + (i == 0 ? lb : 0);
    }
    r.ctx = r.ctxs[0];
    const double took = cw.lap();
    r.tm.ckpt_blocking += took;
    if (r.tm.ckpts++ == 0) r.tm.ckpt_first = took;  // (it pins its buffers; later ones take them back from the writer)
  }
  double waited = 0;
  if (!r.writer.submit(std::move(job), &waited)) {
    r.lerr("%s\n", r.writer.error().c_str());
    exit(-1);
  }
  r.tm.save_wait += waited;
  r.tm.save_blocking += sw.lap();
  r.tm.saves++;
  r.saved_iter = r.iter;
}

// every gamma.txt / theta.txt handed to the writer is complete and closed (before the process ends, on every path)
void finish_saves(Run &r) {
  double waited = 0;
  const bool ok = r.writer.drain(&waited);
  r.tm.save_wait += waited;
  r.tm.save_blocking += waited;
  r.tm.save_writer = r.writer.busy_seconds();
  if (!ok) {
    r.lerr("%s\n", r.writer.error().c_str());
    fprintf(stderr, "%s\n", r.writer.error().c_str());
    r.writer.stop();
    exit(-1);
  }
}

void write_timing(Run &r) {
  FILE *f = fopen(r.file_str("/timing.txt").c_str(), "w");
  if (!f) return;
  const Timing &t = r.tm;
  fprintf(f, "# wall-clock seconds of this run (host/terastructure_main.cpp; not a reference file)\n");
  fprintf(f, "ingest: %.3f\nvalidation sample: %.3f\ninit gamma: %.3f\ntraining: %.3f\nvalidation reports: %.3f (%u)\n", t.ingest, t.validation_sample,
          t.init_gamma, t.training, t.report, t.reports);
  fprintf(f, "save_model, main thread blocked: %.3f (%u saves; of which waiting for the writer: %.3f)\n", t.save_blocking, t.saves, t.save_wait);
  fprintf(f, "save_model, writer thread busy (overlapped with training): %.3f\n", t.save_writer);
  if (r.o.checkpoint)
    fprintf(f, "checkpoint, main thread blocked (part of save_model's): %.3f (%u checkpoints, %.1f MB of engine state each; the first, which pins its buffers: %.3f)\n",
            t.ckpt_blocking, t.ckpts, t.ckpts ? (double)t.ckpt_bytes / t.ckpts / 1e6 : 0.0, t.ckpt_first);
  if (!r.o.resume.empty()) fprintf(f, "resume (read, validate, import): %.3f\n", t.resume);
  if (!r.o.project.empty())
    fprintf(f, "project (load lambda, fold in, foldin.txt): %.3f (%u updates, %u of %u individuals converged)\n", t.project, t.project_iters_run,
            t.project_converged, r.o.n);
  if (r.o.logl) fprintf(f, "training likelihood (-logl): %.3f (%u evaluations)\n", t.logl, t.logls);
  if (!r.o.kinship.empty())
    fprintf(f, "kinship (-kinship): %.3f (%zu individuals, %u pairs listed)\n", t.kinship, r.kin_ids.size(), t.kinship_pairs);
  if (r.o.scan) fprintf(f, "scan (-scan): %.3f (%u locations%s)\n", t.scan, r.o.l, r.o.pheno.empty() ? "" : ", with a trait");
  if (r.o.ld_set)
    fprintf(f, "ld (-ld): %.3f (window %u, %llu pairs listed, %u of %u locations kept)\n", t.ld, r.o.ld, (unsigned long long)t.ld_pairs, t.ld_kept, r.o.l);
  if (r.o.theta_se)
    fprintf(f, "theta standard errors (-theta-se): %.3f (%u individuals, %u not identified)\n", t.theta_se, r.o.n, t.theta_se_na);
  fprintf(f, "total: %u\n", r.duration());
  fclose(f);
}

void kinship(Run &r);  // (-kinship, below)
void scan(Run &r);     // (-scan, below)
void ld(Run &r);       // (-ld, below)
void theta_se(Run &r); // (-theta-se, below)

// -project: the checkpoint's lambda into every context in chunks, tsamd_fold_in over all locations from gamma = 1 (no
// validation sample is drawn: every stored genotype counts), then theta.txt / gamma.txt through the usual writer and
// foldin.txt: individual, updates applied, change of the last one
void project(Run &r, const ckpt::Buf &loc) {
  Stopwatch sw;
  const Options &o = r.o;
  const size_t J = 2 * (size_t)o.k;
  const double *lam = (const double *)(loc.data() + sizeof(ckpt::BlobHeader));  // (128-byte header: as aligned as the buffer)
  const uint32_t chunk = std::max<uint32_t>(1u, (uint32_t)std::min<size_t>(o.l, (64u << 20) / (J * sizeof(double))));
  for (tsamd_ctx *c : r.ctxs) {
    r.ctx = c;
    for (uint32_t l0 = 0; l0 < o.l; l0 += chunk) TS(r, tsamd_set_lambda_range(c, l0, std::min(chunk, o.l - l0), lam + (size_t)l0 * J));
  }
  r.ctx = r.ctxs[0];
  printf("+ projecting %u individuals onto the lambda of %s\n", o.n, o.project.c_str());
  fflush(stdout);
  std::vector<uint32_t> iters(o.n);
  std::vector<double> change(o.n);
  for (size_t i = 0; i < r.ctxs.size(); ++i) {
    uint32_t b, c, conv = 0, ran = 0;
    shard_span(r, i, b, c);
    r.ctx = r.ctxs[i];
    TS(r, tsamd_fold_in(r.ctxs[i], nullptr, o.l, o.project_iters, o.project_tol, iters.data() + b, change.data() + b, &conv, &ran));
    r.tm.project_converged += conv;
    r.tm.project_iters_run = std::max(r.tm.project_iters_run, ran);
  }
  r.ctx = r.ctxs[0];
  r.lerr("projected onto %s: %u updates, %u of %u individuals converged (tol %g)", o.project.c_str(), r.tm.project_iters_run, r.tm.project_converged,
         o.n, o.project_tol);
  save_model(r, false);
  FILE *f = fopen(r.file_str("/foldin.txt").c_str(), "w");
  if (!f) {
    fprintf(stderr, "cannot open foldin.txt: %s\n", strerror(errno));
    exit(-1);
  }
  for (uint32_t n = 0; n < o.n; ++n) fprintf(f, "%u\t%u\t%.8e\n", n, iters[n], change[n]);
  fclose(f);
  r.tm.project = sw.lap();
  if (!o.kinship.empty()) kinship(r);  // (the folded-in theta against the file's lambda)
  if (o.scan) scan(r);                 // likewise
  if (o.ld_set) ld(r);                 // likewise
  if (o.theta_se) theta_se(r);         // likewise: the standard errors of the projected cohort
  finish_saves(r);
  write_timing(r);
  printf("+ done: %u updates, %u of %u individuals converged\n", r.tm.project_iters_run, r.tm.project_converged, o.n);
}

// -kinship: reads the list -- one 0-based individual index per line -- and checks it against -n, TSAMD_KIN_MAX_M and the
// shards of -devices (tsamd_kinship answers for pairs inside one shard); false and a reason when it cannot be used
bool read_kinship_ids(Run &r, std::string *why) {
  const Options &o = r.o;
  FILE *f = fopen(o.kinship.c_str(), "r");
  if (!f) {
    *why = "cannot open " + o.kinship + ": " + strerror(errno);
    return false;
  }
  char line[256];
  uint32_t lineno = 0;
  bool ok = true;
  while (ok && fgets(line, sizeof line, f) != nullptr) {
    ++lineno;
    char *e = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(line, &e, 10);
    const char *q = e;
    while (*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n') ++q;
    if (e == line && *q == 0) continue;  // an empty line
    if (e == line || *q != 0 || errno != 0 || strchr(line, '-') != nullptr || v >= o.n) {
      *why = o.kinship + " line " + std::to_string(lineno) + ": not an individual index below -n " + std::to_string(o.n);
      ok = false;
    } else if (r.kin_ids.size() >= TSAMD_KIN_MAX_M) {
      *why = o.kinship + " lists more than " + std::to_string(TSAMD_KIN_MAX_M) + " individuals";
      ok = false;
    } else
      r.kin_ids.push_back((uint32_t)v);
  }
  fclose(f);
  if (ok && r.kin_ids.empty()) {
    *why = o.kinship + " lists no individual";
    ok = false;
  }
  if (!ok) return false;
  const uint32_t world = (uint32_t)std::max<size_t>(1, o.devices.size());
  for (uint32_t rank = 0; rank < world; ++rank) {
    uint32_t b = 0, c = 0;
    tsamd_shard_range(o.n, rank, world, &b, &c);
    if (r.kin_ids[0] >= b && r.kin_ids[0] - b < c) {
      r.kin_shard = rank;
      for (uint32_t id : r.kin_ids)
        if (id < b || id - b >= c) {
          *why = "individuals " + std::to_string(r.kin_ids[0]) + " and " + std::to_string(id) + " lie on different devices' shards: pairs across shards are not supported";
          return false;
        }
    }
  }
  return true;
}

// -kinship: tsamd_kinship of the listed individuals over all l locations under the state of the final save_model;
// kinship.txt "i \t j \t kin \t den" for the pairs i < j (positions in the list give the order, the file's indices the
// names) with kin >= -kinship-min, inbreeding.txt "i \t 2 kin_ii - 1"; "%.8f" through fmt_fixed8
void kinship(Run &r) {
  Stopwatch sw;
  const Options &o = r.o;
  const uint32_t m = (uint32_t)r.kin_ids.size();
  std::vector<double> kin((size_t)m * m), den((size_t)m * m);
  r.ctx = r.ctxs[r.kin_shard];
  TS(r, tsamd_kinship(r.ctx, r.kin_ids.data(), m, nullptr, o.l, kin.data(), nullptr, den.data()));
  r.ctx = r.ctxs[0];
  FILE *fk = fopen(r.file_str("/kinship.txt").c_str(), "w"), *fi = fopen(r.file_str("/inbreeding.txt").c_str(), "w");
  if (!fk || !fi) {
    r.lerr("cannot open kinship.txt / inbreeding.txt:%s\n", strerror(errno));
    exit(-1);
  }
  std::vector<char> buf((size_t)m * (2 * (tsfmt::kMaxLen + 1) + 32));
  for (uint32_t a = 0; a < m; ++a) {
    char *p = buf.data();
    for (uint32_t b = a + 1; b < m; ++b) {
      const double v = kin[(size_t)a * m + b];
      if (!(v >= o.kinship_min)) continue;
      p = tsfmt::fmt_uint(p, r.kin_ids[a]);
      *p++ = '\t';
      p = tsfmt::fmt_uint(p, r.kin_ids[b]);
      *p++ = '\t';
      p = tsfmt::fmt_fixed8(p, v);
      *p++ = '\t';
      p = tsfmt::fmt_fixed8(p, den[(size_t)a * m + b]);
      *p++ = '\n';
      r.tm.kinship_pairs++;
    }
    fwrite(buf.data(), 1, (size_t)(p - buf.data()), fk);
    p = tsfmt::fmt_uint(buf.data(), r.kin_ids[a]);
    *p++ = '\t';
    p = tsfmt::fmt_fixed8(p, 2.0 * kin[(size_t)a * m + a] - 1.0);
    *p++ = '\n';
    fwrite(buf.data(), 1, (size_t)(p - buf.data()), fi);
  }
  fclose(fk);
  fclose(fi);
  r.tm.kinship += sw.lap();
  r.lerr("kinship of %u individuals: %u pairs at or above %g", m, r.tm.kinship_pairs, o.kinship_min);
}

// -theta-se: the observed information of every individual over all l locations under the state of the final save_model
// (tsamd_theta_info, every device its own shard, -theta-se-rows individuals per call so that the host holds that many rows of
// K (K + 1) / 2 doubles), tsamd_theta_se on each batch; theta_se.txt has one line per individual in theta.txt's order: the K
// standard errors, tab-separated, "%.8f" through fmt_fixed8, NA for every value of a row that is not identified
void theta_se(Run &r) {
  Stopwatch sw;
  const Options &o = r.o;
  const uint32_t K = o.k, P = TSAMD_INFO_PACKED(K);
  FILE *f = fopen(r.file_str("/theta_se.txt").c_str(), "w");
  if (!f) {
    r.lerr("cannot open theta_se.txt:%s\n", strerror(errno));
    exit(-1);
  }
  const uint32_t rows = std::max<uint32_t>(1u, std::min(o.theta_se_rows, o.n));
  std::vector<double> info((size_t)rows * P), se((size_t)rows * K);
  std::vector<uint8_t> status(rows);
  std::vector<uint32_t> ids(rows);
  std::vector<char> buf((size_t)K * (tsfmt::kMaxLen + 1) + 8);
  for (size_t i = 0; i < r.ctxs.size(); ++i) {  // shards in rank order: individuals ascending
    uint32_t b, c;
    shard_span(r, i, b, c);
    r.ctx = r.ctxs[i];
    for (uint32_t n0 = 0; n0 < c; n0 += rows) {
      const uint32_t m = std::min(rows, c - n0);
      for (uint32_t j = 0; j < m; ++j) ids[j] = b + n0 + j;
      // (the shard's first m individuals go without a list: the columns are then read coalesced; the same bits either way)
      TS(r, tsamd_theta_info(r.ctx, n0 == 0 ? nullptr : ids.data(), m, nullptr, o.l, info.data(), nullptr));
      if (tsamd_theta_se(info.data(), m, K, se.data(), nullptr, status.data()) != TSAMD_OK) {
        r.lerr("tsamd_theta_se: %s\n", tsamd_last_error(nullptr));
        exit(-1);
      }
      for (uint32_t j = 0; j < m; ++j) {
        char *p = buf.data();
        for (uint32_t k = 0; k < K; ++k) {
          if (k) *p++ = '\t';
          if (status[j]) {
            *p++ = 'N', *p++ = 'A';
          } else {
            p = tsfmt::fmt_fixed8(p, se[(size_t)j * K + k]);
          }
        }
        *p++ = '\n';
        fwrite(buf.data(), 1, (size_t)(p - buf.data()), f);
        r.tm.theta_se_na += status[j] ? 1u : 0u;
      }
    }
  }
  r.ctx = r.ctxs[0];
  fclose(f);
  r.tm.theta_se += sw.lap();
  r.lerr("standard errors of theta: %u individuals, %u not identified", o.n, r.tm.theta_se_na);
}

// -pheno: reads the trait -- one value per line in theta.txt's order, NA or nan for an individual that is not phenotyped --
// and checks it against -n; false and a reason when it cannot be used
bool read_pheno(Run &r, std::string *why) {
  const Options &o = r.o;
  FILE *f = fopen(o.pheno.c_str(), "r");
  if (!f) {
    *why = "cannot open " + o.pheno + ": " + strerror(errno);
    return false;
  }
  char line[256];
  uint32_t lineno = 0;
  bool ok = true;
  while (ok && fgets(line, sizeof line, f) != nullptr) {
    ++lineno;
    char *b = line;
    while (*b == ' ' || *b == '\t') ++b;
    char *e = b + strlen(b);
    while (e > b && (e[-1] == ' ' || e[-1] == '\t' || e[-1] == '\r' || e[-1] == '\n')) --e;
    *e = 0;
    double v = std::numeric_limits<double>::quiet_NaN();
    if (strcmp(b, "NA") != 0 && strcmp(b, "nan") != 0) {
      char *end = nullptr;
      v = strtod(b, &end);
      if (end == b || *end != 0 || !std::isfinite(v)) {
        *why = o.pheno + " line " + std::to_string(lineno) + ": not a finite number, NA or nan";
        ok = false;
      }
    }
    if (ok && r.pheno.size() >= o.n) {
      *why = o.pheno + " line " + std::to_string(lineno) + ": more lines than -n " + std::to_string(o.n);
      ok = false;
    }
    if (ok) r.pheno.push_back(v);
  }
  fclose(f);
  if (ok && r.pheno.size() != o.n) {
    *why = o.pheno + " has " + std::to_string(r.pheno.size()) + " lines, -n is " + std::to_string(o.n);
    ok = false;
  }
  return ok;
}

// -scan: tsamd_snp_scan over all l locations under the state of the final save_model, the trait sliced by shard and the
// shards' rows added in shard order; every z and p from tsamd_scan_statistics.  scan.txt, one line per location:
// "loc \t n \t O0 \t O1 \t O2 \t E0 \t E1 \t E2 \t z_het \t p_het \t z_freq \t p_freq" and with -pheno "\t n_t \t z_trait \t p_trait"
void scan(Run &r) {
  Stopwatch sw;
  const Options &o = r.o;
  const uint32_t l = o.l;
  const bool trait = !o.pheno.empty();
  std::vector<double> fs((size_t)l * TSAMD_SCAN_FIT_SUMS, 0.0), ts(trait ? (size_t)l * TSAMD_SCAN_TRAIT_SUMS : 0, 0.0), s1(fs.size()), t1(ts.size());
  std::vector<uint32_t> fc((size_t)l * TSAMD_SCAN_FIT_COUNTS, 0u), tc(trait ? l : 0, 0u), c1(fc.size()), n1(tc.size());
  for (size_t i = 0; i < r.ctxs.size(); ++i) {  // shard after shard; no exchange is involved
    uint32_t b, c;
    shard_span(r, i, b, c);
    r.ctx = r.ctxs[i];
    TS(r, tsamd_snp_scan(r.ctxs[i], nullptr, l, trait ? r.pheno.data() + b : nullptr, s1.data(), c1.data(), trait ? t1.data() : nullptr,
                         trait ? n1.data() : nullptr));
    for (size_t x = 0; x < fs.size(); ++x) fs[x] += s1[x];
    for (size_t x = 0; x < fc.size(); ++x) fc[x] += c1[x];
    for (size_t x = 0; x < ts.size(); ++x) ts[x] += t1[x];
    for (size_t x = 0; x < tc.size(); ++x) tc[x] += n1[x];
  }
  r.ctx = r.ctxs[0];
  std::vector<double> st((size_t)l * TSAMD_SCAN_STATS);
  if (tsamd_scan_statistics(fs.data(), fc.data(), trait ? ts.data() : nullptr, trait ? tc.data() : nullptr, l, st.data()) != 0) {
    r.lerr("tsamd_scan_statistics: %s\n", tsamd_last_error(nullptr));
    exit(-1);
  }
  FILE *f = fopen(r.file_str("/scan.txt").c_str(), "w");
  if (!f) {
    r.lerr("cannot open scan.txt:%s\n", strerror(errno));
    exit(-1);
  }
  for (uint32_t j = 0; j < l; ++j) {
    const double *s = &fs[(size_t)j * TSAMD_SCAN_FIT_SUMS], *z = &st[(size_t)j * TSAMD_SCAN_STATS];
    const uint32_t *c = &fc[(size_t)j * TSAMD_SCAN_FIT_COUNTS];
    fprintf(f, "%u\t%u\t%u\t%u\t%u\t%.8f\t%.8f\t%.8f\t%.6f\t%.6e\t%.6f\t%.6e", j, c[0] + c[1] + c[2], c[0], c[1], c[2], s[0], s[1], s[2], z[0], z[1],
            z[2], z[3]);
    if (trait) fprintf(f, "\t%u\t%.6f\t%.6e", tc[j], z[4], z[5]);
    fputc('\n', f);
  }
  fclose(f);
  r.tm.scan += sw.lap();
  r.lerr("scan of %u locations%s", l, trait ? " with a trait" : "");
}

// -ld: tsamd_ld over all l locations under the state of the final save_model.  The locations go in blocks of rows (-ld-rows)
// with an overlap of the window -- by default what the host holds of a block's band, 40 bytes per entry of [rows + window]
// [window + 1] (the sum of num and cnt over the shards, one shard's, r and p), stays under 256 MB, or is 4096 rows -- and the shards'
// bands are added in shard order; r and p from tsamd_ld_statistics.  ld.txt, one line per pair i < j <= i + window with
// r^2 >= -ld-min: "i \t j \t r \t r2 \t n \t p".  The pruning is tsamd_ld_prune's rule carried across the blocks: rows in
// ascending order, a row that is still kept drops the later locations whose r^2 with it exceeds -ld-r2.  prune.in / prune.out:
// one 0-based location per line.
void ld(Run &r) {
  Stopwatch sw;
  const Options &o = r.o;
  const uint32_t l = o.l, w = o.ld, w1 = w + 1u;
  const uint64_t entry = 4u * sizeof(double) + 2u * sizeof(uint32_t), fit = (256ull << 20) / ((uint64_t)w1 * entry);
  const uint32_t rows_max =  // (by default whole internal chunks of the library)
      (uint32_t)std::min<uint64_t>(l, o.ld_rows ? o.ld_rows : std::max<uint64_t>(4096u, fit / 4096u * 4096u));
  FILE *f = fopen(r.file_str("/ld.txt").c_str(), "w"), *fin = fopen(r.file_str("/prune.in").c_str(), "w"), *fout = fopen(r.file_str("/prune.out").c_str(), "w");
  if (!f || !fin || !fout) {
    r.lerr("cannot open ld.txt / prune.in / prune.out:%s\n", strerror(errno));
    exit(-1);
  }
  std::vector<uint8_t> dropped(l, 0);
  std::vector<uint32_t> locs;
  std::vector<double> num, n1, rr, pp;
  std::vector<uint32_t> cnt, c1;
  for (uint32_t b0 = 0; b0 < l; b0 += rows_max) {
    const uint32_t rows = std::min(rows_max, l - b0), n_locs = rows + std::min(w, l - b0 - rows);  // the block's rows and their overlap
    const size_t count = (size_t)n_locs * w1;
    locs.resize(n_locs);
    for (uint32_t i = 0; i < n_locs; ++i) locs[i] = b0 + i;
    num.assign(count, 0.0), cnt.assign(count, 0u), n1.resize(count), c1.resize(count), rr.resize(count), pp.resize(count);
    for (size_t i = 0; i < r.ctxs.size(); ++i) {  // shard after shard; no exchange is involved
      r.ctx = r.ctxs[i];
      TS(r, tsamd_ld(r.ctxs[i], locs.data(), n_locs, w, n1.data(), c1.data()));
      for (size_t x = 0; x < count; ++x) num[x] += n1[x], cnt[x] += c1[x];
    }
    r.ctx = r.ctxs[0];
    if (tsamd_ld_statistics(num.data(), cnt.data(), n_locs, w, rr.data(), pp.data()) != 0) {
      r.lerr("tsamd_ld_statistics: %s\n", tsamd_last_error(nullptr));
      exit(-1);
    }
    for (uint32_t i = 0; i < rows; ++i) {  // (the overlap's rows belong to the next block: their windows are cut short here)
      const uint32_t gi = b0 + i;
      for (uint32_t d = 1; d <= w && gi + d < l; ++d) {
        const size_t x = (size_t)i * w1 + d;
        const double r2 = rr[x] * rr[x];
        if (!dropped[gi] && r2 > o.ld_r2) dropped[gi + d] = 1;
        if (!(r2 >= o.ld_min)) continue;
        fprintf(f, "%u\t%u\t%.8f\t%.8f\t%u\t%.6e\n", gi, gi + d, rr[x], r2, cnt[x], pp[x]);
        r.tm.ld_pairs++;
      }
      fprintf(dropped[gi] ? fout : fin, "%u\n", gi);
      r.tm.ld_kept += dropped[gi] ? 0u : 1u;
    }
  }
  fclose(f);
  fclose(fin);
  fclose(fout);
  r.tm.ld += sw.lap();
  r.lerr("ld of %u locations, window %u: %llu pairs at or above r2 %g, %u locations kept at r2 <= %g", l, w, (unsigned long long)r.tm.ld_pairs, o.ld_min,
         r.tm.ld_kept, o.ld_r2);
}

// compute_likelihood(first, validation = true) (src/snpsamplinge.cc:461-544);
// returns true when the stop rule fires
bool compute_likelihood(Run &r, bool first) {
  uint32_t k = 0;
  double s = .0;
  // The whole block at once (tsamd_heldout_eval): theta is frozen while it runs, so the
  // reference's "per location: optimize_lambda in hol mode, _iter++, held-out sum" is one
  // hol-mode schedule over the validation locations (ascending, the map's order) followed by
  // one evaluation kernel per shard; the sums are then added in the reference's order.
  std::vector<uint32_t> locs;
  locs.reserve(r.validation.size());
  for (auto &kv : r.validation) locs.push_back(kv.first);
  const uint32_t nl = (uint32_t)locs.size();
  if (!first && nl) {  // snp_likelihood: optimize_lambda(loc) in hol mode, then _iter++
    run_all(r, locs.data(), nl, 1);
    r.iter += nl;
  }
  std::vector<std::vector<double>> sums(r.ctxs.size(), std::vector<double>(nl));
  std::vector<std::vector<uint32_t>> cnts(r.ctxs.size(), std::vector<uint32_t>(nl));
  for (size_t i = 0; i < r.ctxs.size(); ++i) {
    r.ctx = r.ctxs[i];
    TS(r, tsamd_heldout_eval(r.ctxs[i], locs.data(), nl, 0, sums[i].data(), cnts[i].data(), nullptr, nullptr));
  }
  r.ctx = r.ctxs[0];
  for (uint32_t j = 0; j < nl; ++j)
    for (size_t i = 0; i < r.ctxs.size(); ++i) {  // ascending individuals: shard after shard
      s += sums[i][j];
      k += cnts[i][j];
    }
  printf("\rdone:%.2f%%", 100.0);
  fprintf(r.vf, "%d\t%d\t%.9f\t%d\t%f\n", r.iter, r.duration(), (s / k), k, exp(s / k));
  fflush(r.vf);
  const double a = s / k;
  bool stop = false;
  if (r.iter > 2000) {
    if (a > r.prev_h && r.prev_h != 0 && fabs((a - r.prev_h) / r.prev_h) < r.o.stop_threshold)
      stop = true;
    else if (a < r.prev_h)
      r.nh++;
    else if (a > r.prev_h)
      r.nh = 0;
    if (a > r.max_h) r.max_h = a;
    if (r.nh > 3) stop = true;
  }
  r.prev_h = a;
  return stop;
}

// -logl: the log-likelihood of the training data under the current state (tsamd_train_loglik: every stored entry of all l
// columns on every shard; held-out entries are not training data).  What the reference announces ("+ computing initial
// training likelihood", the likelihood-analysis.txt it unlinks, src/snpsamplinge.cc:533-534 commented out) and never
// computes.  Every report appends "iter \t secs \t mean \t count \t exp(mean)" to likelihood-analysis.txt; with the final
// save_model (per_entry) the call writes logl_snp.txt ("loc \t count \t mean") and logl_indiv.txt ("count \t mean", theta.txt's
// order) instead.
void train_likelihood(Run &r, bool per_entry) {
  Stopwatch sw;
  const uint32_t l = r.o.l, n = r.o.n;
  std::vector<double> loc_sum, indiv_sum, ls;
  std::vector<uint64_t> loc_cnt;
  std::vector<uint32_t> indiv_cnt, lc;
  if (per_entry) {
    loc_sum.assign(l, 0.0), loc_cnt.assign(l, 0), ls.resize(l), lc.resize(l);
    indiv_sum.assign(n, 0.0), indiv_cnt.assign(n, 0);
  }
  double total = 0.0;
  uint64_t count = 0;
  for (size_t i = 0; i < r.ctxs.size(); ++i) {  // shard after shard; no exchange is involved
    uint32_t b, c;
    shard_span(r, i, b, c);
    double s = 0.0;
    uint64_t m = 0;
    r.ctx = r.ctxs[i];
    TS(r, tsamd_train_loglik(r.ctxs[i], nullptr, l, per_entry ? ls.data() : nullptr, per_entry ? lc.data() : nullptr,
                             per_entry ? indiv_sum.data() + b : nullptr, per_entry ? indiv_cnt.data() + b : nullptr, &s, &m));
    total += s;
    count += m;
    if (per_entry)
      for (uint32_t j = 0; j < l; ++j) loc_sum[j] += ls[j], loc_cnt[j] += lc[j];
  }
  r.ctx = r.ctxs[0];
  if (!per_entry) {
    const double mean = count ? total / (double)count : 0.0;
    FILE *f = fopen(r.file_str("/likelihood-analysis.txt").c_str(), "a");
    if (!f) {
      r.lerr("cannot open likelihood-analysis.txt:%s\n", strerror(errno));
      exit(-1);
    }
    fprintf(f, "%d\t%d\t%.9f\t%llu\t%f\n", r.iter, r.duration(), mean, (unsigned long long)count, exp(mean));
    fclose(f);
  } else {
    FILE *fs = fopen(r.file_str("/logl_snp.txt").c_str(), "w"), *fi = fopen(r.file_str("/logl_indiv.txt").c_str(), "w");
    if (!fs || !fi) {
      r.lerr("cannot open logl_snp.txt / logl_indiv.txt:%s\n", strerror(errno));
      exit(-1);
    }
    for (uint32_t j = 0; j < l; ++j)
      fprintf(fs, "%u\t%llu\t%.8f\n", j, (unsigned long long)loc_cnt[j], loc_cnt[j] ? loc_sum[j] / (double)loc_cnt[j] : 0.0);
    for (uint32_t i = 0; i < n; ++i) fprintf(fi, "%u\t%.8f\n", indiv_cnt[i], indiv_cnt[i] ? indiv_sum[i] / (double)indiv_cnt[i] : 0.0);
    fclose(fs);
    fclose(fi);
  }
  r.tm.logl += sw.lap();
  r.tm.logls++;
}

void save_beta(Run &r, const std::vector<uint32_t> *locs) {
  const size_t k = r.o.k;
  FILE *f = fopen(add_iter_suffix(r, "/beta").c_str(), "w");
  if (!f) {
    r.lerr("cannot open beta or lambda file:%s\n", strerror(errno));
    exit(-1);
  }
  // "%d\t" loc, K x "%.8f\t", "\n" (src/snpsamplinge.cc:761-798) -- through fmt_fixed8, a block of rows per fwrite
  const uint32_t chunk = 1u << 16;
  std::vector<double> eb((size_t)chunk * k);
  std::vector<char> buf;
  auto put_rows = [&](const uint32_t *ids, uint32_t first, uint32_t nl) {
    buf.resize((size_t)nl * (k * (tsfmt::kMaxLen + 1) + 16));
    char *p = buf.data();
    for (uint32_t j = 0; j < nl; ++j) {
      p = tsfmt::fmt_uint(p, ids ? ids[j] : first + j);
      *p++ = '\t';
      for (size_t q = 0; q < k; ++q) {
        p = tsfmt::fmt_fixed8(p, eb[(size_t)j * k + q]);
        *p++ = '\t';
      }
      *p++ = '\n';
    }
    if (fwrite(buf.data(), 1, (size_t)(p - buf.data()), f) != (size_t)(p - buf.data())) {
      r.lerr("error writing beta file:%s\n", strerror(errno));
      exit(-1);
    }
  };
  if (!locs) {
    for (uint32_t l0 = 0; l0 < r.o.l; l0 += chunk) {
      const uint32_t nl = std::min(chunk, r.o.l - l0);
      TS(r, tsamd_get_ebeta(r.ctx, l0, nl, eb.data()));
      put_rows(nullptr, l0, nl);
    }
  } else {
    for (uint32_t loc : *locs) {
      TS(r, tsamd_get_ebeta(r.ctx, loc, 1, eb.data()));
      put_rows(&loc, 0, 1);
    }
  }
  fclose(f);
}

// SNP::read_idfile (src/snp.cc:255-276): one whitespace-separated label per individual, in order
void read_idfile(Run &r) {
  FILE *f = fopen(r.o.idfile.c_str(), "r");
  if (!f) {
    r.lerr("cannot open file %s:%s", r.o.idfile.c_str(), strerror(errno));
    fprintf(stderr, "error reading %s; quitting\n", r.o.idfile.c_str());
    exit(-1);
  }
  char tok[128];
  while (fscanf(f, "%127s", tok) == 1) r.labels.push_back(tok);
  fclose(f);
}

// load_gamma (src/snpsamplinge.cc:800-862): ./gamma.txt of the CURRENT directory
void load_gamma(Run &r) {
  const size_t n = r.o.n, k = r.o.k;
  FILE *gf = fopen("gamma.txt", "r");
  if (!gf) {
    r.lerr("cannot open gamma file:%s\n", strerror(errno));
    fprintf(stderr, "cannot open gamma file:%s\n", strerror(errno));
    exit(-1);
  }
  std::vector<double> g(n * k, 1.0);
  const int sz = 128 * (int)k;
  std::vector<char> line(sz);
  size_t row = 0;
  while (row < n && fgets(line.data(), sz, gf) != nullptr) {
    char *p = line.data();
    for (size_t j = 0; j < k; ++j) {
      char *q = nullptr;
      const double d = strtod(p, &q);
      if (p == q) {
        fprintf(stderr, "error parsing gamma file\n");
        exit(-1);
      }
      g[row * k + j] = d;
      p = q;
    }
    row++;
  }
  fclose(gf);
  if (row != n) {
    fprintf(stderr, "gamma.txt has %zu rows, expected %zu\n", row, n);
    exit(-1);
  }
  set_gamma_all(r, g);
  FILE *f = fopen(r.file_str("/gammasave.txt").c_str(), "w");
  if (f) {  // (id, label, K x "%.8f\t", argmax: src/snpsamplinge.cc:846-860 -- the values through fmt_fixed8, the bytes of "%.8f")
    std::vector<char> line(k * (tsfmt::kMaxLen + 1) + 1);
    for (size_t i = 0; i < n; ++i) {
      fprintf(f, "%zu\t%s\t", i, (i < r.labels.size() && !r.labels[i].empty()) ? r.labels[i].c_str() : "unknown");
      double mx = .0;
      size_t mk = 0;
      char *p = line.data();
      for (size_t j = 0; j < k; ++j) {
        p = tsfmt::fmt_fixed8(p, g[i * k + j]);
        *p++ = '\t';
        if (g[i * k + j] > mx) mx = g[i * k + j], mk = j;
      }
      fwrite(line.data(), 1, (size_t)(p - line.data()), f);
      fprintf(f, "%zu\n", mk);
    }
    fclose(f);
  }
}

void run_batch(Run &r, const std::vector<uint32_t> &locs) {
  run_all(r, locs.data(), (uint32_t)locs.size(), 0);
}

}  // namespace

int main(int argc, char **argv) {
  signal(SIGTERM, term_handler);
  Run r;
  Options &o = r.o;
  if (argc == 1) {
    usage();
    exit(-1);
  }
  for (int i = 1; i < argc; ++i) {
    auto need = [&](const char *flag) -> const char * {
      if (i + 1 > argc - 1) {
        fprintf(stderr, "+ insufficient arguments for %s!\n", flag);
        exit(-1);
      }
      return argv[++i];
    };
    const char *a = argv[i];
    if (!strcmp(a, "-help")) {
      usage();
      exit(0);
    } else if (!strcmp(a, "-force")) {
      fprintf(stdout, "+ overwrite option set\n");
      o.force = true;
    } else if (!strcmp(a, "-online") || !strcmp(a, "-E") || !strcmp(a, "-stochastic")) {
      fprintf(stdout, "+ stochastic option set\n");
    } else if (!strcmp(a, "-file") || !strcmp(a, "-bed")) {
      o.datfname = need(a);
      fprintf(stdout, "+ using file %s\n", o.datfname.c_str());
    } else if (!strcmp(a, "-bfile")) {
      o.datfname = std::string(need(a)) + ".bed";
      fprintf(stdout, "+ using file %s\n", o.datfname.c_str());
    } else if (!strcmp(a, "-batch")) {
      fprintf(stdout, "batch option currently not available");
      exit(0);
    } else if (!strcmp(a, "-n")) {
      o.n = atoi(need(a));
      fprintf(stdout, "+ n = %d\n", o.n);
    } else if (!strcmp(a, "-k")) {
      o.k = atoi(need(a));
      fprintf(stdout, "+ K = %d\n", o.k);
    } else if (!strcmp(a, "-l")) {
      o.l = atoi(need(a));
      fprintf(stdout, "+ L = %d\n", o.l);
    } else if (!strcmp(a, "-label")) {
      o.label = need(a);
    } else if (!strcmp(a, "-eta-type")) {
      o.eta_type = need(a);
    } else if (!strcmp(a, "-rfreq")) {
      o.rfreq = atoi(need(a));
      o.rfreq_set = true;
      fprintf(stdout, "+ rfreq = %d\n", o.rfreq);
    } else if (!strcmp(a, "-logl")) {
      o.logl = true;
    } else if (!strcmp(a, "-idfile")) {
      o.idfile = need(a);  // labels are only echoed into gammasave.txt by the reference
      fprintf(stdout, "+ idfile = %s\n", o.idfile.c_str());
    } else if (!strcmp(a, "-loadcmp")) {
      o.loadcmp = true;
    } else if (!strcmp(a, "-seed")) {
      o.seed = atof(need(a));
      fprintf(stdout, "+ random seed set to %.5f\n", o.seed);
    } else if (!strcmp(a, "-file-suffix")) {
      o.file_suffix = true;
    } else if (!strcmp(a, "-save-beta")) {
      o.save_beta = true;
    } else if (!strcmp(a, "-adagrad")) {
      o.adagrad = true;
    } else if (!strcmp(a, "-nthreads")) {
      o.nthreads = atoi(need(a));  // accepted; the GPU replaces the worker threads
    } else if (!strcmp(a, "-use-test-set")) {
      o.use_test_set = true;  // broken in the reference (writes to an unopened FILE*); ignored
    } else if (!strcmp(a, "-locations-file")) {
      o.locations_file = need(a);
    } else if (!strcmp(a, "-compute-beta")) {
      o.compute_beta = true;
    } else if (!strcmp(a, "-stop-threshold")) {
      o.stop_threshold = atof(need(a));
    } else if (!strcmp(a, "-device")) {
      o.device = atoi(need(a));
    } else if (!strcmp(a, "-devices")) {
      o.devices.clear();
      for (const char *q = need(a); *q;) {
        char *e = nullptr;
        o.devices.push_back((int)strtol(q, &e, 10));
        if (e == q) {
          fprintf(stdout, "error: -devices expects a comma separated list of device ordinals\n");
          exit(-1);
        }
        q = (*e == ',') ? e + 1 : e;
      }
    } else if (!strcmp(a, "-max-iter")) {
      o.max_iter = atoi(need(a));
    } else if (!strcmp(a, "-ingest-threads")) {
      o.ingest_threads = (unsigned)atoi(need(a));
    } else if (!strcmp(a, "-ingest-only")) {
      o.ingest_only = true;
    } else if (!strcmp(a, "-checkpoint")) {
      o.checkpoint = true;
    } else if (!strcmp(a, "-resume")) {
      o.resume = need(a);
    } else if (!strcmp(a, "-project")) {
      o.project = need(a);
    } else if (!strcmp(a, "-project-iters")) {
      o.project_iters = (uint32_t)atoi(need(a));
    } else if (!strcmp(a, "-project-tol")) {
      o.project_tol = atof(need(a));
    } else if (!strcmp(a, "-kinship")) {
      o.kinship = need(a);
    } else if (!strcmp(a, "-kinship-min")) {
      o.kinship_min = atof(need(a));
    } else if (!strcmp(a, "-scan")) {
      o.scan = true;
    } else if (!strcmp(a, "-pheno")) {
      o.pheno = need(a);
    } else if (!strcmp(a, "-ld")) {
      o.ld = (uint32_t)std::max(0, atoi(need(a)));
      o.ld_set = true;
    } else if (!strcmp(a, "-ld-r2")) {
      o.ld_r2 = atof(need(a));
    } else if (!strcmp(a, "-ld-min")) {
      o.ld_min = atof(need(a));
    } else if (!strcmp(a, "-ld-rows")) {
      o.ld_rows = (uint32_t)std::max(0, atoi(need(a)));
      o.ld_rows_set = true;
    } else if (!strcmp(a, "-theta-se")) {
      o.theta_se = true;
    } else if (!strcmp(a, "-theta-se-rows")) {
      o.theta_se_rows = (uint32_t)std::max(0, atoi(need(a)));
    } else {
      fprintf(stdout, "error: unknown option %s\n", a);
      exit(-1);
    }
  }
  if (!o.rfreq_set) o.rfreq = 100000;
  if (o.n == 0 || o.l == 0 || o.k == 0) {
    fprintf(stderr, "error: -n, -l and -k are required\n");
    exit(-1);
  }
  if (o.loadcmp) {
    fprintf(stdout, "+ loadcmp option set: nothing to do\n");
    return 0;
  }

  if (!o.project.empty() && (!o.resume.empty() || o.compute_beta)) {
    fprintf(stderr, "error: -project fits a cohort against a trained model; it does not go with %s\n", o.compute_beta ? "-compute-beta" : "-resume");
    return -1;
  }
  // -resume: the file is read and checked against the flags before anything else exists -- a checkpoint of another run,
  // a truncated or a corrupt one is refused with nothing written (the engine validates its parts once more on import)
  ckpt::FileHeader resume_head{};
  ckpt::HostState resume_host{};
  ckpt::Buf resume_loc, resume_indiv;
  Stopwatch resume_sw;
  if (!o.resume.empty()) {
    if (o.compute_beta) {
      fprintf(stderr, "error: -resume continues a training run; it does not go with -compute-beta\n");
      return -1;
    }
    std::string why;
    const ckpt::Expect want{o.n, o.l, o.k, o.rfreq, o.seed};
    if (!ckpt::read_file(o.resume, want, &resume_head, &resume_host, &resume_loc, &resume_indiv, &why)) {
      fprintf(stderr, "error: -resume: %s\n", why.c_str());
      return -1;
    }
    r.tm.resume = resume_sw.lap();
  }

  // -project: likewise -- the file's lambda is read and checked against -l / -k before anything else exists
  ckpt::FileHeader project_head{};
  ckpt::Buf project_loc;
  if (!o.project.empty()) {
    if (o.project_iters == 0 || !(o.project_tol >= 0.0) || !std::isfinite(o.project_tol)) {
      fprintf(stderr, "error: -project-iters must be positive, -project-tol finite and not negative\n");
      return -1;
    }
    std::string why;
    if (!ckpt::read_loc_part(o.project, o.l, o.k, &project_head, &project_loc, &why)) {
      fprintf(stderr, "error: -project: %s\n", why.c_str());
      return -1;
    }
  }

  // -kinship: the list is read and checked before anything else exists
  if (!o.kinship.empty()) {
    if (o.compute_beta || o.ingest_only) {
      fprintf(stderr, "error: -kinship evaluates a run's final model; it does not go with %s\n", o.compute_beta ? "-compute-beta" : "-ingest-only");
      return -1;
    }
    std::string why;
    if (!read_kinship_ids(r, &why)) {
      fprintf(stderr, "error: -kinship: %s\n", why.c_str());
      return -1;
    }
  }

  // -scan / -pheno: the trait is read and checked before anything else exists
  if (!o.pheno.empty() && !o.scan) {
    fprintf(stderr, "error: -pheno gives -scan its trait; it needs -scan\n");
    return -1;
  }
  if (o.scan) {
    if (o.compute_beta || o.ingest_only) {
      fprintf(stderr, "error: -scan evaluates a run's final model; it does not go with %s\n", o.compute_beta ? "-compute-beta" : "-ingest-only");
      return -1;
    }
    std::string why;
    if (!o.pheno.empty() && !read_pheno(r, &why)) {
      fprintf(stderr, "error: -pheno: %s\n", why.c_str());
      return -1;
    }
  }

  // -ld: the window and the thresholds are checked before anything else exists
  if (o.ld_set) {
    if (o.compute_beta || o.ingest_only) {
      fprintf(stderr, "error: -ld evaluates a run's final model; it does not go with %s\n", o.compute_beta ? "-compute-beta" : "-ingest-only");
      return -1;
    }
    if (o.ld == 0 || o.ld > TSAMD_LD_MAX_WINDOW || !(o.ld_r2 >= 0.0) || !std::isfinite(o.ld_r2) || !std::isfinite(o.ld_min)) {
      fprintf(stderr, "error: -ld needs a window of 1 to %d locations, -ld-r2 finite and not negative, -ld-min finite\n", TSAMD_LD_MAX_WINDOW);
      return -1;
    }
    if (o.ld_rows_set && o.ld_rows == 0) {
      fprintf(stderr, "error: -ld-rows needs at least 1 location\n");
      return -1;
    }
  }

  // -theta-se: likewise
  if (o.theta_se) {
    if (o.compute_beta || o.ingest_only) {
      fprintf(stderr, "error: -theta-se evaluates a run's final model; it does not go with %s\n", o.compute_beta ? "-compute-beta" : "-ingest-only");
      return -1;
    }
    if (o.theta_se_rows == 0) {
      fprintf(stderr, "error: -theta-se-rows needs at least 1 individual\n");
      return -1;
    }
  }

  // the GPU context comes first so that a missing device fails before any output exists
  tsamd_config cfg;
  tsamd_default_config(&cfg, o.n, o.l, o.k);
  if (o.compute_beta) cfg.max_inner = 100;  // tightly optimize given the thetas (:75)
  if (o.devices.empty()) o.devices.push_back(o.device);
  cfg.world = (uint32_t)o.devices.size();
  for (size_t i = 0; i < o.devices.size(); ++i) {
    cfg.device = o.devices[i];
    cfg.rank = (uint32_t)i;
    tsamd_ctx *c = nullptr;
    if (tsamd_create(&cfg, &c) != 0) {
      fprintf(stderr, "error: tsamd_create: %s\n", tsamd_last_error(nullptr));
      return -1;
    }
    r.ctxs.push_back(c);
  }
  r.ctx = r.ctxs[0];
  if (r.ctxs.size() > 1 && tsamd_p2p_connect_local(r.ctxs.data(), (uint32_t)r.ctxs.size()) != 0) {
    fprintf(stderr, "error: tsamd_p2p_connect_local: %s\n", tsamd_last_error(r.ctx));
    return -1;
  }

  setup_run_dir(r);
  Stopwatch phase;
  {  // SNP::read (src/snp.cc:9-21): the extension decides
    const std::string ext = o.datfname.size() >= 4 ? o.datfname.substr(o.datfname.size() - 4) : "";
    if (ext == ".bed") {
      printf("+ bed format detected\n");
      read_bed(r);
    } else if (ext == ".012") {
      read_012(r);
    } else {
      r.lerr("unrecognized file extension");
      fprintf(stderr, "unrecognized file extension\n");
      exit(-1);
    }
  }
  r.tm.ingest = phase.lap();
  if (o.ingest_only) {
    write_timing(r);
    destroy_all(r);
    return 0;
  }
  if (o.idfile != "") read_idfile(r);  // (src/main.cc:208)
  printf("+ initialization begin\n");
  fflush(stdout);
  r.plog_u("individuals n", o.n);
  r.plog_u("locations l", o.l);
  r.plog_u("populations k", o.k);

  if (!o.project.empty()) {
    project(r, project_loc);
    destroy_all(r);
    return 0;
  }

  Mt19937 rng(0);  // gsl_rng_alloc: default seed 0 -> 4357
  if (o.seed) rng.set((unsigned long)o.seed);
  r.rng = &rng;
  unlink(r.file_str("/likelihood-analysis.txt").c_str());
  r.vf = fopen(r.file_str("/validation.txt").c_str(), "w");
  if (!r.vf) {
    printf("cannot open heldout file:%s\n", strerror(errno));
    exit(-1);
  }

  if (o.compute_beta) {
    set_validation_sample(r, rng);
    r.lerr("done starting threads");
    load_gamma(r);
    r.lerr("done estimating all theta");
    std::vector<uint32_t> locs;
    if (o.locations_file == "") {
      locs.resize(o.l);
      for (uint32_t i = 0; i < o.l; ++i) locs[i] = i;
    } else {
      FILE *f = fopen(o.locations_file.c_str(), "r");
      if (!f) {
        fprintf(stderr, "cannot open %s\n", o.locations_file.c_str());
        exit(-1);
      }
      char line[16384];
      while (fgets(line, sizeof line, f) != nullptr) {
        unsigned v;
        if (sscanf(line, "%u", &v) == 1 && v < o.l) locs.push_back(v);
      }
      fclose(f);
    }
    // compute_all_lambda (:368-381): the same hot path per location, gamma steps included
    const size_t chunk = 4096;
    for (size_t i0 = 0; i0 < locs.size(); i0 += chunk) {
      std::vector<uint32_t> part(locs.begin() + i0, locs.begin() + std::min(locs.size(), i0 + chunk));
      run_batch(r, part);
      r.iter += (uint32_t)part.size();
      printf("\rloc = %d took %d secs", r.iter, r.duration());
      fflush(stdout);
    }
    save_beta(r, o.locations_file == "" ? nullptr : &locs);
    destroy_all(r);
    return 0;
  }

  phase.lap();
  set_validation_sample(r, rng);
  r.tm.validation_sample = phase.lap();
  if (!o.resume.empty()) {
    // instead of init_gamma, the initial likelihood and the initial save: the engine state of the file into every shard
    // (the location part as it is, the shard's slice of the global individual part), then the host's own -- the
    // generator's state replaces the one the validation sample has just advanced (the sample itself is a function of
    // the seed and the data: it came out as in the run that wrote the file)
    resume_sw.lap();
    for (size_t i = 0; i < r.ctxs.size(); ++i) {
      uint32_t b, c;
      shard_span(r, i, b, c);
      ckpt::Buf part;
      std::string why;
      if (!ckpt::slice_indiv(resume_indiv.data(), resume_indiv.size(), b, c, &part, &why)) {
        fprintf(stderr, "error: -resume: %s\n", why.c_str());
        exit(-1);
      }
      r.ctx = r.ctxs[i];
      TS(r, tsamd_state_import(r.ctxs[i], part.data(), part.size(), resume_loc.data(), resume_loc.size()));
    }
    r.ctx = r.ctxs[0];
    r.iter = resume_host.iter;
    r.nh = resume_host.nh;
    r.prev_h = resume_host.prev_h;
    r.max_h = resume_host.max_h;
    memcpy(rng.mt, resume_host.mt, sizeof rng.mt);
    rng.mti = resume_host.mti;
    r.tm.resume += resume_sw.lap();
    r.lerr("resumed from %s at iteration %u", o.resume.c_str(), r.iter);
    printf("+ resumed from %s at iteration %u\n", o.resume.c_str(), r.iter);
    resume_loc.alloc(0);
    resume_indiv.alloc(0);
  } else {
    {  // init_gamma (:226-237): n-major, k inner, Gamma(100 v, 0.01)
      std::vector<double> g((size_t)o.n * o.k);
      for (size_t i = 0; i < g.size(); ++i) {
        const double v = (o.k < 100) ? 1.0 : (double)100.0 / o.k;
        g[i] = rng.gamma(100 * v, 0.01);
      }
      set_gamma_all(r, g);
    }
    r.tm.init_gamma = phase.lap();
    printf("+ computing initial heldout likelihood\n");
    compute_likelihood(r, true);
    r.tm.report += phase.lap();
    r.tm.reports++;
    if (o.logl) train_likelihood(r, false);
    save_model(r, false);  // (the initial state: nothing to resume from yet)
  }
  printf("\n+ computing initial training likelihood\n+ done..\n+ initialization end\n");
  fflush(stdout);

  // infer() (:417-459).  Locations are drawn one per iteration from the same stream; they
  // are data-independent, so a whole report period is enqueued at once.
  while (true) {
    uint32_t c = o.rfreq - (r.iter % o.rfreq);
    c = std::min<uint32_t>(c, 4096);  // bounds the latency of a SIGTERM
    if (o.max_iter && r.iter + c > o.max_iter) c = o.max_iter > r.iter ? o.max_iter - r.iter : 0;
    std::vector<uint32_t> locs(c);
    for (uint32_t i = 0; i < c; ++i) locs[i] = rng.uniform_int(o.l);
    phase.lap();
    if (c) run_batch(r, locs);
    r.tm.training += phase.lap();
    r.iter += c;
    printf("\riteration = %d took %d secs", r.iter, r.duration());
    fflush(stdout);
    if (c && r.iter % o.rfreq == 0) {
      printf("iteration = %d took %d secs\n", r.iter, r.duration());
      r.lerr("iteration = %d took %d secs\n", r.iter, r.duration());
      r.lerr("computing heldout likelihood @ %d secs", r.duration());
      phase.lap();
      const bool stop = compute_likelihood(r, false);
      r.tm.report += phase.lap();
      r.tm.reports++;
      if (o.logl) train_likelihood(r, false);
      if (stop) {
        save_model(r);
        break;
      }
      r.lerr("saving theta @ %d secs", r.duration());
      save_model(r);
      r.lerr("done @ %d secs", r.duration());
    }
    if (g_terminate || (o.max_iter && r.iter >= o.max_iter)) {
      // (a report that ended at this very iteration has just saved this state: the same bytes would be written again)
      if (r.saved_iter != r.iter) save_model(r);
      break;
    }
  }
  printf("\n");
  if (o.logl) train_likelihood(r, true);  // the state of the final save_model: the per-location and per-individual files
  if (!o.kinship.empty()) kinship(r);     // likewise
  if (o.scan) scan(r);                    // likewise
  if (o.ld_set) ld(r);                    // likewise
  if (o.theta_se) theta_se(r);            // likewise
  finish_saves(r);  // gamma.txt / theta.txt complete and closed before the process ends
  write_timing(r);
  destroy_all(r);
  return 0;
}
