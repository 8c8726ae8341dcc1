// tsamd_snp_scan: per-location sufficient statistics of the structure-adjusted fit and association tests (gfx950).
//
// With q = sum_k Ebeta[j][k] Etheta[n][k], h = 2q(1-q) and r = y - 2q, every stored entry of a listed column adds
// (1-q)^2, h, q^2, h(1-h) and its genotype class to the location's fit sums and, where the individual carries a trait value t,
// t, t r, t^2 h, t h, r and h to its trait sums (scan_add_entry, tsamd_scan_plan.h).  The host turns the sums into z and p
// (scan_statistics_row).  Reads the state, writes none of it; no per-individual output.
//
// Tile.  The tile of ts_loglik<K>: a workgroup of 256 threads takes tile_n = 256 IPT consecutive individuals; a thread takes
// IPT consecutive ones (scan_ipt) and keeps their normalised theta -- gamma / sum_k gamma, divided ONCE when the workgroup
// starts -- in IPT K <= 64 doubles (128 VGPRs) for all the locations it visits, with their trait values (0 in place of NaN)
// and phenotyped masks beside them.  Per location a thread reads the ONE 32-bit word of the 2-bit column that holds its
// individuals (the word of the next location is requested before the arithmetic of the current one) and forms the IPT
// values of q with K FMAs each.  Ebeta = lambda0 / (lambda0 + lambda1) of kScanBatch locations at a time is computed once per
// workgroup into LDS.  The stored-entry mask and the phenotyped mask are factors 0 or 1: the sweep has no branch on the
// data, no log, no division and no exp.
// K above TSAMD_SPECIALIZED_K runs the same kernel with a run-time K (template argument 0): one individual per thread, theta
// read per entry from a normalised [K][npad] array that ts_loglik_theta fills once per call.
//
// Summation order (no floating-point atomics).  Per location: a thread adds its IPT terms in ascending order onto zeros, the
// wave adds its 64 lanes for all 7 / 14 values at once with the fixed butterfly of WaveFold<8> / WaveFold<16> (the lowest lane
// of a slot), the four waves' values are added in ascending order through LDS and stored as the tile's partial in
// part [len][ntiles][values]; ts_scan_finish adds a location's tiles in ascending order.  Nothing in that order depends on the
// other locations of the call, on the segment or on the chunk a location falls in.  The counts ride the same fold as doubles:
// every partial is an integer below 2^24, every total one below 2^32, so they are exact; ts_scan_finish converts them.
//
// Scratch memory: part takes at most kScanScratchBound = 256 MB (scan_geometry cuts a long list into chunks of locations
// accordingly); it is allocated on first use and freed by tsamd_destroy.
//
// Per location and individual: 2 bits of genotype read (N / 4 bytes a location: the only stream from HBM); 2 K flops for q,
// 17 for the fit terms and their sums, 3 conversions, and with a trait 15 more: about 2 K + 25 with a trait.
// Measured once on one MI355X (2026-10-19, tools/scan_rate.py, profiles/scan_rates.md), with / without a trait: 2.34 / 1.39 us per
// location at N = 1M, K = 8 (ts_loglik in the same build: 4.21); 1.73 / 1.12 us at N = 500K, K = 16; 0.58 / 0.40 us at N = 125K, K = 20.
#pragma once
#include "tsamd_device.h"
#include "tsamd_scan_plan.h"

namespace tsamd {

template <int KC, bool TRAIT>
__global__ __launch_bounds__(256) void ts_scan(const ScanArgs a) {
  constexpr int IPT = (int)scan_ipt((uint32_t)KC, TRAIT);
  constexpr int KMAX = KC > 0 ? KC : TSAMD_MAX_K;
  constexpr int NV = (int)scan_values(TRAIT);
  using Fold = WaveFold<NV>;
  constexpr int P = Fold::P;
  __shared__ double s_eb[kScanBatch * KMAX];
  __shared__ uint32_t s_loc[kScanBatch];
  __shared__ double s_part[4][kScanBatch][P];
  const uint32_t K = KC > 0 ? (uint32_t)KC : a.K;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = blockIdx.x, seg = blockIdx.y;
  const uint32_t n0 = tile * (uint32_t)(kScanBlock * IPT) + tid * (uint32_t)IPT;  // this thread's first individual
  const bool active = n0 < a.npad;  // (npad is a multiple of 512 and of IPT: a thread's individuals are all inside or all outside)
  const uint32_t word = n0 >> 4, shift = 2u * (n0 & 15u);
  // after the fold the lanes 0, 4, 8, ... hold the wave's total of value slot(lane) (the lowest lane of each slot)
  const int my_slot = Fold::slot(lane);
  const bool writer = (lane & (uint32_t)(64 / P - 1)) == 0u;

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
  // the trait: 0 in place of NaN, and the phenotyped mask as a factor
  double tv[IPT], pm[IPT];
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    tv[i] = 0.0, pm[i] = 0.0;
    if constexpr (TRAIT) {
      const double t = active ? a.trait[n0 + i] : 0.0;
      const bool has = active && t == t;
      tv[i] = has ? t : 0.0;
      pm[i] = has ? 1.0 : 0.0;
    }
  }

  const uint32_t b_begin = seg * a.seg_len, b_end = min(a.len, b_begin + a.seg_len);
  for (uint32_t b0 = b_begin; b0 < b_end; b0 += kScanBatch) {
    const uint32_t nb = min(kScanBatch, b_end - b0);
    __syncthreads();  // (the previous batch's partials have been read)
    if (tid < nb) s_loc[tid] = a.locs[b0 + tid];
    for (uint32_t e = tid; e < nb * K; e += kScanBlock) {
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
      double v[P];
#pragma unroll
      for (int x = 0; x < P; ++x) v[x] = 0.0;
#pragma unroll
      for (int i = 0; i < IPT; ++i) scan_add_entry<TRAIT>(q[i], (codes >> (2 * i)) & 3u, tv[i], pm[i], v);
      const double total = Fold::fold(v, lane);
      if (writer) s_part[wave][j][my_slot] = total;
    }
    __syncthreads();
    for (uint32_t e = tid; e < nb * (uint32_t)NV; e += kScanBlock) {
      const uint32_t j = e / (uint32_t)NV, x = e - j * (uint32_t)NV;
      double s = 0.0;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) s += s_part[wv][j][x];
      a.part[((size_t)(b0 + j) * a.ntiles + tile) * NV + x] = s;
    }
  }
}

// a location's tiles, in ascending order; one thread per (location, value).  out_sums [len][10]: the fit sums, then the
// trait sums (0 without a trait); out_counts [len][4]: y = 0, 1, 2, then the phenotyped entries
__global__ __launch_bounds__(256) void ts_scan_finish(const double *part, uint32_t len, uint32_t ntiles, uint32_t values, double *out_sums,
                                                      uint32_t *out_counts) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= len * (uint32_t)kScanTraitValues) return;
  const uint32_t i = e / (uint32_t)kScanTraitValues, x = e - i * (uint32_t)kScanTraitValues;
  double s = 0.0;
  if (x < values)
    for (uint32_t t = 0; t < ntiles; ++t) s += part[((size_t)i * ntiles + t) * values + x];
  if (x < (uint32_t)kScanO0)
    out_sums[(size_t)i * 10u + x] = s;
  else if (x < (uint32_t)kScanFitValues)
    out_counts[(size_t)i * 4u + (x - (uint32_t)kScanO0)] = (uint32_t)s;
  else if (x < (uint32_t)kScanNT)
    out_sums[(size_t)i * 10u + 4u + (x - (uint32_t)kScanT)] = s;
  else
    out_counts[(size_t)i * 4u + 3u] = (uint32_t)s;
}

}  // namespace tsamd
