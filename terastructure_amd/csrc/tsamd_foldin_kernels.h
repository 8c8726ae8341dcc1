// tsamd_fold_in: fit the individuals' gamma against a FIXED lambda (gfx950) -- projecting a cohort onto a trained panel.
//
// One update of individual n over the listed locations J (tsamd_foldin_plan.h; the batch form of update_gamma /
// update_phimom / update_phidad, src/snpsamplinge.cc:627-647, :696-719, with rho = 1):
//   S0_j = sum_k w_k eb[j][k][0],  S1_j = sum_k w_k eb[j][k][1]
//   acc_k = sum_{j in J, code != 01}  y eb[j][k][0] / S0_j + (2 - y) eb[j][k][1] / S1_j
//   gamma'_k = alpha + w_k acc_k,   change = mean_k |gamma'_k - gamma_k| / mean_k gamma'_k
// w = exp(Elogtheta) up to a factor per individual, which cancels in w_k / S: the array the engine keeps (DevParams::w).
// Linear domain throughout: 4 K multiply-adds and two reciprocals per entry, no exp or log in the sweep.
//
// Sweep, ts_foldin_sweep<K>, K = 1 .. 32.  A workgroup of 256 threads takes tile_n = 256 IPT consecutive individuals; a
// thread takes IPT consecutive ones, IPT = 16 / 8 / 4 / 2 / 1 at K <= 2 / 4 / 8 / 16 / 32 (foldin_ipt), and keeps their w
// and acc -- 2 IPT K <= 64 doubles, 128 VGPRs -- in registers for every location it visits.  Per location a thread
// reads the ONE 32-bit word of the 2-bit column that holds its individuals (the word of the next location is requested
// before the arithmetic of the current one).  exp(Elogbeta) of kFoldinBatch locations at a time is copied once per
// workgroup into LDS; the waves read it by broadcast (moved to SGPRs with uniform_f64 where enough multiply-adds share a
// value to pay for the two moves).  Grid (tiles, segments): when the tiles are fewer than the compute units the list is
// cut into segments (foldin_geometry) -- a few thousand individuals against a million locations.  Each (segment, k,
// individual) writes ONE partial; a workgroup whose tile has no active individual left returns at once.
// K above 32, ts_foldin_sweep_wide: a run-time K, one individual per thread, w read from the [K][npad] array; per batch of
// kFoldinWideBatch locations the 2 x 16 coefficients y / S0_j, (2 - y) / S1_j are formed in registers (loop over k outside,
// one load of w_k for the 16 locations), then for every k the batch's contribution is added to acc_k in the partials
// array itself: one read-modify-write per k and batch, by the owning thread (the segment's first batch writes).
//
// Step, ts_foldin_step, one thread per individual: adds the segments' partials in ascending order, forms gamma', the
// change, the frozen flag and the iteration count, computes the new w as ts_refresh_w does (exp_digamma_split,
// exp_nonpos), counts the individuals still active with an integer atomic (one per wave) and flags their tiles.  Frozen
// and padding individuals are not touched.
//
// Summation order (no floating-point atomics): a thread adds an individual's entries in the listed order over its
// segment, the step adds the segments in ascending order.  Nothing depends on another individual, so a result is the
// same bits whatever the other individuals do; it depends on the segment count (rounding only).
//
// Scratch memory: the partials [nseg][K][npad], at most 256 MB or the size of gamma itself, whichever is larger
// (foldin_scratch_bound caps the segment count), and 16 bytes per individual; allocated on first use, freed by tsamd_destroy.
#pragma once
#include "tsamd_device.h"
#include "tsamd_foldin_plan.h"

namespace tsamd {

template <int KC>
__global__ __launch_bounds__(256) void ts_foldin_sweep(const FoldinArgs a) {
  static_assert(KC >= 1 && KC <= (int)kFoldinSpecializedK, "K = 1 .. 32; ts_foldin_sweep_wide serves the rest");
  constexpr int IPT = (int)foldin_ipt((uint32_t)KC);
  __shared__ double s_eb[kFoldinBatch * 2 * KC];
  __shared__ uint32_t s_loc[kFoldinBatch];
  const uint32_t tid = threadIdx.x;
  const uint32_t tile = blockIdx.x, seg = blockIdx.y;
  if (a.active[1u + tile] == 0u) return;  // (the whole workgroup: every individual of the tile is frozen)
  const uint32_t n0 = tile * (uint32_t)(kFoldinBlock * IPT) + tid * (uint32_t)IPT;  // this thread's first individual
  const bool inside = n0 < a.npad;  // (npad is a multiple of 512 and of IPT: a thread's individuals are all inside or all outside)
  const uint32_t word = n0 >> 4, shift = 2u * (n0 & 15u);

  double w[IPT][KC], acc[IPT][KC];
#pragma unroll
  for (int i = 0; i < IPT; ++i)
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      w[i][k] = inside ? a.w[(size_t)k * a.npad + n0 + i] : 1.0;
      acc[i][k] = 0.0;
    }

  const uint32_t b_begin = seg * a.seg_len, b_end = min(a.n_locs, b_begin + a.seg_len);
  for (uint32_t b0 = b_begin; b0 < b_end; b0 += kFoldinBatch) {
    const uint32_t nb = min(kFoldinBatch, b_end - b0);
    __syncthreads();  // (the previous batch has been read)
    if (tid < nb) s_loc[tid] = a.locs ? a.locs[b0 + tid] : b0 + tid;
    for (uint32_t e = tid; e < nb * 2u * KC; e += kFoldinBlock) {
      const uint32_t j = e / (2u * KC), r = e - j * (2u * KC);
      const uint32_t loc = a.locs ? a.locs[b0 + j] : b0 + j;
      s_eb[e] = a.eb[(size_t)loc * (2u * KC) + r];
    }
    __syncthreads();
    auto load_word = [&](uint32_t j) -> uint32_t {
      const uint32_t loc = __builtin_amdgcn_readfirstlane(s_loc[j]);
      const uint32_t *col = reinterpret_cast<const uint32_t *>(a.bed + (size_t)loc * a.colstride);
      return inside ? col[word] : 0x55555555u;  // (outside the shard's padded width: all missing)
    };
    uint32_t w_next = load_word(0u);
    for (uint32_t j = 0; j < nb; ++j) {
      const uint32_t codes = w_next >> shift;
      if (j + 1u < nb) w_next = load_word(j + 1u);
      const double *ebj = s_eb + j * 2u * KC;
      double s0[IPT], s1[IPT];
#pragma unroll
      for (int i = 0; i < IPT; ++i) s0[i] = 0.0, s1[i] = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const double2 v = *reinterpret_cast<const double2 *>(ebj + 2 * k);
        const double e0 = IPT >= 4 ? uniform_f64(v.x) : v.x, e1 = IPT >= 4 ? uniform_f64(v.y) : v.y;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
          s0[i] = fma(w[i][k], e0, s0[i]);
          s1[i] = fma(w[i][k], e1, s1[i]);
        }
      }
      double c0[IPT], c1[IPT];
#pragma unroll
      for (int i = 0; i < IPT; ++i) foldin_coeffs(s0[i], s1[i], (codes >> (2 * i)) & 3u, c0[i], c1[i]);
      // (K >= 29: the second loop reads exp(Elogbeta) from LDS again instead of keeping the first loop's 2 K values live
      // beside w and acc, which would take the thread past 256 VGPRs)
      if constexpr (KC >= 29) asm volatile("" ::: "memory");
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const double2 v = *reinterpret_cast<const double2 *>(ebj + 2 * k);
        const double e0 = IPT >= 4 ? uniform_f64(v.x) : v.x, e1 = IPT >= 4 ? uniform_f64(v.y) : v.y;
#pragma unroll
        for (int i = 0; i < IPT; ++i) acc[i][k] = fma(c0[i], e0, fma(c1[i], e1, acc[i][k]));
      }
    }
  }
  if (inside) {
    double *part = a.part + (size_t)seg * KC * a.npad + n0;
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int i = 0; i < IPT; ++i) part[(size_t)k * a.npad + i] = acc[i][k];
  }
}

// run-time K (33 .. 128): one individual per thread
__global__ __launch_bounds__(256) void ts_foldin_sweep_wide(const FoldinArgs a) {
  constexpr uint32_t B = kFoldinWideBatch;
  __shared__ double s_eb[B * 2 * kFoldinMaxK];
  __shared__ uint32_t s_loc[B];
  const uint32_t tid = threadIdx.x, K = a.K;
  const uint32_t tile = blockIdx.x, seg = blockIdx.y;
  if (a.active[1u + tile] == 0u) return;
  const uint32_t n = tile * kFoldinBlock + tid;
  const bool inside = n < a.npad;
  const uint32_t nn = inside ? n : 0u;  // (threads outside the padded width compute on individual 0 and store nothing)
  const uint32_t word = nn >> 4, shift = 2u * (nn & 15u);
  const double *wn = a.w + nn;
  double *part = a.part + (size_t)seg * K * a.npad + nn;

  const uint32_t b_begin = seg * a.seg_len, b_end = min(a.n_locs, b_begin + a.seg_len);
  for (uint32_t b0 = b_begin; b0 < b_end; b0 += B) {
    const uint32_t nb = min(B, b_end - b0);
    __syncthreads();
    if (tid < B) s_loc[tid] = tid < nb ? (a.locs ? a.locs[b0 + tid] : b0 + tid) : 0xffffffffu;
    for (uint32_t e = tid; e < B * 2u * K; e += kFoldinBlock) {
      const uint32_t j = e / (2u * K), r = e - j * (2u * K);
      double v = 1.0;  // (past the end of the list: any positive value, the codes there read as missing)
      if (j < nb) {
        const uint32_t loc = a.locs ? a.locs[b0 + j] : b0 + j;
        v = a.eb[(size_t)loc * (2u * K) + r];
      }
      s_eb[e] = v;
    }
    __syncthreads();
    uint32_t code[B];
#pragma unroll
    for (uint32_t j = 0; j < B; ++j) {
      const uint32_t loc = __builtin_amdgcn_readfirstlane(s_loc[j]);
      uint32_t c = 0x55555555u;
      if (loc != 0xffffffffu && inside) c = reinterpret_cast<const uint32_t *>(a.bed + (size_t)loc * a.colstride)[word];
      code[j] = (c >> shift) & 3u;
    }
    double c0[B], c1[B];
#pragma unroll
    for (uint32_t j = 0; j < B; ++j) c0[j] = 0.0, c1[j] = 0.0;
    for (uint32_t k = 0; k < K; ++k) {
      const double wk = wn[(size_t)k * a.npad];
#pragma unroll
      for (uint32_t j = 0; j < B; ++j) {
        const double2 v = *reinterpret_cast<const double2 *>(s_eb + (j * K + k) * 2u);
        c0[j] = fma(wk, v.x, c0[j]);
        c1[j] = fma(wk, v.y, c1[j]);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < B; ++j) foldin_coeffs(c0[j], c1[j], code[j], c0[j], c1[j]);
    const bool first = b0 == b_begin;
    for (uint32_t k = 0; k < K; ++k) {
      double v = first || !inside ? 0.0 : part[(size_t)k * a.npad];
#pragma unroll
      for (uint32_t j = 0; j < B; ++j) {
        const double2 e = *reinterpret_cast<const double2 *>(s_eb + (j * K + k) * 2u);
        v = fma(c0[j], e.x, fma(c1[j], e.y, v));
      }
      if (inside) part[(size_t)k * a.npad] = v;
    }
  }
}

// before the first update
__global__ __launch_bounds__(256) void ts_foldin_init(const FoldinArgs a) {
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  if (n < a.npad) {
    a.iters[n] = 0u;
    a.change[n] = 0.0;
    a.frozen[n] = n < a.n_local ? 0u : 1u;
  }
  if (n == 0u) a.active[0] = a.n_local;
  if (n < a.ntiles) a.active[1u + n] = (uint64_t)n * a.tile_n < a.n_local ? 1u : 0u;
}

// one thread per individual; a.active has been zeroed
__global__ __launch_bounds__(256) void ts_foldin_step(const FoldinArgs a) {
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  bool still = false;
  if (n < a.n_local && a.frozen[n] == 0u) {
    const uint32_t K = a.K;
    const size_t np = a.npad;
    double sum_abs = 0.0, sum_new = 0.0;
    for (uint32_t k = 0; k < K; ++k) {
      double acc = 0.0;
      for (uint32_t g = 0; g < a.nseg; ++g) acc += a.part[((size_t)g * K + k) * np + n];  // ascending segments
      const double old = a.gam[(size_t)k * np + n];
      const double nw = foldin_gamma(a.alpha, a.w[(size_t)k * np + n], acc);
      a.gam[(size_t)k * np + n] = nw;
      sum_abs += fabs(nw - old);
      sum_new += nw;
    }
    const double change = foldin_change(sum_abs, sum_new);
    a.iters[n] += 1u;
    a.change[n] = change;
    still = !(change < a.tol);
    if (!still) a.frozen[n] = 1u;
    // w = exp(psi(gamma)) up to a factor, as ts_refresh_w_wide forms it
    double amax = -1.0e300;
    for (uint32_t k = 0; k < K; ++k) {
      double z, e;
      exp_digamma_split(a.gam[(size_t)k * np + n], z, e);
      amax = fmax(amax, e);
    }
    for (uint32_t k = 0; k < K; ++k) {
      double z, e;
      exp_digamma_split(a.gam[(size_t)k * np + n], z, e);
      a.w[(size_t)k * np + n] = z * exp_nonpos(e - amax);
    }
  }
  const unsigned long long m = __ballot(still);
  if (m != 0ull && (threadIdx.x & 63u) == 0u) {
    atomicAdd(&a.active[0], (uint32_t)__popcll(m));
    a.active[1u + n / a.tile_n] = 1u;  // (tile_n is a multiple of 256: a wave lies in one tile; every writer stores the same 1)
  }
}

}  // namespace tsamd
