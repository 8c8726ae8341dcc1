// tsamd_train_loglik: the training-data log-likelihood of the current state, per location and per individual (gfx950).
//
// term(n, j) = log(max(C(2,y) q^y (1-q)^(2-y), 1e-30)),  q = sum_k Ebeta[j][k] Etheta[n][k]  (tsamd_loglik_plan.h; the term
// of snp_likelihood, src/snpsamplinge.hh:336-360, that heldout_term restates for a few thousand held-out entries), here for
// every stored entry of the listed columns in one sweep.  Reads the state, writes none of it.
//
// Tile.  A workgroup of 256 threads takes tile_n = 256 IPT consecutive individuals; a thread takes IPT consecutive ones,
// IPT = 16 / 8 / 4 / 2 at K <= 4 / 8 / 16 / 32 (loglik_ipt), and keeps their normalised theta -- gamma / sum_k gamma, divided
// ONCE when the workgroup starts -- in IPT K <= 64 doubles (128 VGPRs) for all the locations it visits.  Per location a thread
// reads the ONE 32-bit word of the 2-bit column that holds its individuals (16 / IPT neighbouring lanes read the same word: a
// wave reads 4 IPT contiguous bytes, a workgroup 64 IPT; the word of the next location is requested before the arithmetic of
// the current one), forms the IPT values of q with K FMAs each, picks the product by y and takes one log per entry.
// Ebeta = lambda0 / (lambda0 + lambda1) of kLoglikBatch locations at a time is computed once per workgroup into LDS; the
// waves read it by broadcast (moved to SGPRs with uniform_f64 where enough FMAs share a value to pay for the two moves).
// K above TSAMD_SPECIALIZED_K runs the same kernel with a run-time K (template argument 0): one individual per thread, theta
// read per entry from a normalised [K][npad] array that ts_loglik_theta fills once per call.
//
// Summation order (no floating-point atomics).  Per location: a thread adds its IPT terms in ascending order, the wave
// adds its 64 lanes with the fixed butterfly of WaveFold<1> (lane 0's value), thread j adds the four waves' values in
// ascending order and stores the tile's partial sum in row j of part_loc [len][ntiles]; ts_loglik_finish_loc adds a row's
// tiles in ascending order.  Nothing in that order depends on the other locations of the call, on the segment or on the
// chunk a location falls in.  Per individual: a thread adds its terms in the listed order over its segment and stores them
// in row seg of part_ind [nseg][npad]; ts_loglik_finish_indiv adds the segments in ascending order onto the call's
// accumulator, chunk after chunk.  Counts are integers (wave ballots and popcounts) and take the same route.
//
// Scratch memory: the partial-sum buffers take at most kLoglikScratchBound = 256 MB (loglik_geometry cuts a long list into
// chunks of locations accordingly); they are allocated on first use and freed by tsamd_destroy.
//
// Per location and individual: 2 bits of genotype read (N / 4 bytes a location: the only stream from HBM, 0.25 MB at N = 1M);
// 2 K flops for q, 3 for the product, 2 additions and one library log (a few dozen fp64 instructions): 2 K + 5 + one log.
// Measured once on one MI355X (2026-10-19, tools/train_loglik_rate.py, profiles/train_loglik_rates.md): 4.20 us per location at
// N = 1M, K = 8; 2.48 us at N = 500K, K = 16; 0.75 us at N = 125K, K = 20 -- bound by the fp64 arithmetic of the log.
#pragma once
#include "tsamd_device.h"
#include "tsamd_loglik_plan.h"

namespace tsamd {

template <int KC>
__global__ __launch_bounds__(256) void ts_loglik(const LoglikArgs a) {
  constexpr int IPT = (int)loglik_ipt((uint32_t)KC);
  constexpr int KMAX = KC > 0 ? KC : TSAMD_MAX_K;
  __shared__ double s_eb[kLoglikBatch * KMAX];
  __shared__ uint32_t s_loc[kLoglikBatch];
  __shared__ double s_sum[4][kLoglikBatch];
  __shared__ uint32_t s_cnt[4][kLoglikBatch];
  const uint32_t K = KC > 0 ? (uint32_t)KC : a.K;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = blockIdx.x, seg = blockIdx.y;
  const uint32_t n0 = tile * (uint32_t)(kLoglikBlock * IPT) + tid * (uint32_t)IPT;  // this thread's first individual
  const bool active = n0 < a.npad;  // (npad is a multiple of 512 and of IPT: a thread's individuals are all inside or all outside)
  const uint32_t word = n0 >> 4, shift = 2u * (n0 & 15u);

  // normalised theta of the thread's individuals, exactly what tsamd_get_theta returns: gamma / (sum in ascending k)
  double th[IPT][KC > 0 ? KC : 1];
  if constexpr (KC > 0) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        th[i][k] = active ? a.gam[(size_t)k * a.npad + n0 + i] : 1.0;
        s += th[i][k];
      }
#pragma unroll
      for (int k = 0; k < KC; ++k) th[i][k] = th[i][k] / s;
    }
  }

  double isum[IPT];
  uint32_t icnt[IPT];
#pragma unroll
  for (int i = 0; i < IPT; ++i) isum[i] = 0.0, icnt[i] = 0u;

  const uint32_t b_begin = seg * a.seg_len, b_end = min(a.len, b_begin + a.seg_len);
  for (uint32_t b0 = b_begin; b0 < b_end; b0 += kLoglikBatch) {
    const uint32_t nb = min(kLoglikBatch, b_end - b0);
    __syncthreads();  // (the previous batch's partials have been read)
    if (tid < nb) s_loc[tid] = a.locs[b0 + tid];
    for (uint32_t e = tid; e < nb * K; e += kLoglikBlock) {
      const uint32_t j = e / K, k = e - j * K;
      const double2 l = reinterpret_cast<const double2 *>(a.lam)[(size_t)a.locs[b0 + j] * K + k];
      double s = 0.0;  // (as ts_export_loc adds them)
      s += l.x;
      s += l.y;
      s_eb[e] = l.x / s;
    }
    __syncthreads();
    auto load_word = [&](uint32_t j) -> uint32_t {
      const uint32_t loc = __builtin_amdgcn_readfirstlane(s_loc[j]);
      const uint32_t *col = reinterpret_cast<const uint32_t *>(a.bed + (size_t)loc * a.colstride);
      return active ? col[word] : 0x55555555u;  // (outside the shard's padded width: all missing)
    };
    uint32_t w_next = load_word(0u);
    for (uint32_t j = 0; j < nb; ++j) {
      const uint32_t codes = w_next >> shift;
      if (j + 1u < nb) w_next = load_word(j + 1u);
      double q[IPT];
#pragma unroll
      for (int i = 0; i < IPT; ++i) q[i] = 0.0;
      if constexpr (KC > 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const double v = s_eb[j * KC + k];
          const double e = IPT >= 4 ? uniform_f64(v) : v;  // (two moves to SGPRs per value: not worth it for two FMAs)
#pragma unroll
          for (int i = 0; i < IPT; ++i) q[i] = fma(e, th[i][k], q[i]);
        }
      } else {
        const double *t = a.thn + (active ? n0 : 0u);
        for (uint32_t k = 0; k < K; ++k) q[0] = fma(s_eb[j * K + k], t[(size_t)k * a.npad], q[0]);
      }
      double lsum[1] = {0.0};
      uint32_t wcnt = 0u;
#pragma unroll
      for (int i = 0; i < IPT; ++i) {
        const uint32_t c = (codes >> (2 * i)) & 3u;
        const bool ok = loglik_code_ok(c);
        const double t = ok ? loglik_term(q[i], loglik_code_y(c)) : 0.0;
        isum[i] += t;
        icnt[i] += ok ? 1u : 0u;
        lsum[0] += t;
        wcnt += (uint32_t)__popcll(__ballot(ok));
      }
      const double wsum = WaveFold<1>::fold(lsum, lane);
      if (lane == 0u) s_sum[wave][j] = wsum, s_cnt[wave][j] = wcnt;
    }
    __syncthreads();
    if (tid < nb) {
      double s = 0.0;
      uint32_t c = 0u;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) s += s_sum[wv][tid], c += s_cnt[wv][tid];
      a.part_loc_sum[(size_t)(b0 + tid) * a.ntiles + tile] = s;
      a.part_loc_cnt[(size_t)(b0 + tid) * a.ntiles + tile] = c;
    }
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      a.part_ind_sum[(size_t)seg * a.npad + n0 + i] = isum[i];
      a.part_ind_cnt[(size_t)seg * a.npad + n0 + i] = icnt[i];
    }
  }
}

// run-time-K path: thn [K][npad] = gamma / sum_k gamma, what tsamd_get_theta returns
__global__ __launch_bounds__(256) void ts_loglik_theta(const double *gam, uint32_t npad, uint32_t K, double *thn) {
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  if (n >= npad) return;
  double s = 0.0;
  for (uint32_t k = 0; k < K; ++k) s += gam[(size_t)k * npad + n];
  for (uint32_t k = 0; k < K; ++k) thn[(size_t)k * npad + n] = gam[(size_t)k * npad + n] / s;
}

// a location's tiles, in ascending order
__global__ __launch_bounds__(256) void ts_loglik_finish_loc(const double *part_sum, const uint32_t *part_cnt, uint32_t len, uint32_t ntiles,
                                                            double *out_sum, uint32_t *out_cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= len) return;
  double s = 0.0;
  uint32_t c = 0u;
  for (uint32_t t = 0; t < ntiles; ++t) s += part_sum[(size_t)i * ntiles + t], c += part_cnt[(size_t)i * ntiles + t];
  out_sum[i] = s;
  out_cnt[i] = c;
}

// an individual's segments, in ascending order, onto the call's accumulator
__global__ __launch_bounds__(256) void ts_loglik_finish_indiv(const double *part_sum, const uint32_t *part_cnt, uint32_t nseg, uint32_t npad,
                                                              double *acc_sum, uint32_t *acc_cnt) {
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  if (n >= npad) return;
  double s = acc_sum[n];
  uint32_t c = acc_cnt[n];
  for (uint32_t g = 0; g < nseg; ++g) s += part_sum[(size_t)g * npad + n], c += part_cnt[(size_t)g * npad + n];
  acc_sum[n] = s;
  acc_cnt[n] = c;
}

}  // namespace tsamd
