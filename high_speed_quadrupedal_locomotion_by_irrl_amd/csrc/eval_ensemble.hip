// eval_ensemble.hip -- the ensemble analysis of a body recorder (irrl_eval_ensemble, include/irrl_env.h): one workgroup per (analysed frame,
// condition) turns the condition's E recorder rows into cell keys (csrc/eval_elements.hpp), sorts them in LDS and reads entropy, cell counts,
// per-feature histograms and moments off the sorted array.  A translation unit of its own, compiled by the plain driver; no global atomics
// and no floating-point atomics: every output word has exactly one writer.
//
// Order of the work in a workgroup of 1024 threads (16 waves):
//   1. samples: thread t takes explorations t, t + 1024, ...: features, key (the all-ones sentinel for a dropped sample), LDS integer atomics
//      into the six histograms, per-thread f64 sums of x and x^2;
//   2. the sums go through a fixed tree: xor-butterfly over the 64 lanes of a wave, then the 16 waves added in index order by one thread;
//   3. bitonic sort of the P = 2^ceil(log2 E) keys, ascending, the sentinels end up behind the M kept keys.  Pair i of a pass with stride j is
//      (lo, lo + j), lo = 2 i - (i mod j): for j >= 32 the 32 lanes of a half-wave read 32 consecutive 8-byte words, all 64 banks once; for
//      j < 32 they span 128 dwords, a 2-way conflict on the reads (the stores are bound by their register transfer, not by the array);
//   4. runs of equal keys: a run starts at i where key[i] != key[i - 1]; an inclusive max-scan of (start ? i : -1) gives every position its
//      run's first index, so a run's length is read at its LAST element as i - start + 1 -- no thread ever walks a run, whatever its length.
//      The scan goes round by round over 1024 consecutive positions: shuffles inside a wave, the 16 wave totals through LDS (two buffers, one
//      barrier per round), a running carry between rounds;
//   5. -(n / M) log(n / M) per run end, added per thread in round order, then through the tree of step 2: the sum's order depends on the sorted
//      keys, P and the workgroup size only, so the entropy is the same bits under any permutation of the explorations.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eval_ensemble.hpp"

#define ENS_THREADS 1024
#define ENS_WAVES (ENS_THREADS / 64)
#define ENS_SENTINEL 0xFFFFFFFFFFFFFFFFull

// sum over the 64 lanes of a wave, the same order in every lane
static __device__ __forceinline__ double ens_wave_sum(double v) {
  for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(ENS_THREADS) void irrl_eval_ensemble_kernel(const EnsembleArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ens_lds[];
  uint64_t *keys = reinterpret_cast<uint64_t *>(ens_lds);                       // [P]
  __shared__ unsigned int hist_s[IRRL_EVAL_ENSEMBLE_DIM * IRRL_EVAL_ENSEMBLE_MAX_BINS];
  __shared__ double sum_s[ENS_WAVES][2 * IRRL_EVAL_ENSEMBLE_DIM];
  __shared__ double h_s[ENS_WAVES];
  __shared__ unsigned int runs_s[ENS_WAVES][2];
  __shared__ int scan_s[2][ENS_WAVES];
  __shared__ unsigned int kept_s;

  const int f = (int)blockIdx.x, c = (int)blockIdx.y, tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int E = a.E, P = a.P;
  const int bins = a.hist ? a.spec.hist_bins : 0;
  const size_t cell = (size_t)c * (size_t)a.F + (size_t)f;

  for (int i = tid; i < IRRL_EVAL_ENSEMBLE_DIM * bins; i += ENS_THREADS) hist_s[i] = 0u;
  for (int i = E + tid; i < P; i += ENS_THREADS) keys[i] = ENS_SENTINEL;
  if (tid == 0) kept_s = 0u;
  __syncthreads();

  // 1. samples
  const size_t env0 = (size_t)c * (size_t)E;
  const size_t row0 = (size_t)((long long)a.frame_first + (long long)f * (long long)a.frame_every) * (size_t)a.N + env0;
  double sx[IRRL_EVAL_ENSEMBLE_DIM], sxx[IRRL_EVAL_ENSEMBLE_DIM];
  for (int i = 0; i < IRRL_EVAL_ENSEMBLE_DIM; i++) { sx[i] = 0.0; sxx[i] = 0.0; }
  for (int e = tid; e < E; e += ENS_THREADS) {
    uint64_t key = ENS_SENTINEL;
    if (!a.mask || a.mask[env0 + (size_t)e] != 0) {
      double x[IRRL_EVAL_ENSEMBLE_DIM];
      irrl_eval_ensemble_features(a.rec_body + (row0 + (size_t)e) * 13, x);
      uint64_t k;
      if (irrl_eval_ensemble_key(x, a.spec, &k)) {
        key = k;
        for (int i = 0; i < IRRL_EVAL_ENSEMBLE_DIM; i++) {
          const double xx = x[i] * x[i];
          sx[i] += x[i];
          sxx[i] += xx;
          if (bins > 0) {
            const int b = irrl_eval_ensemble_bin(x[i], a.spec.hist_lo[i], a.spec.hist_hi[i], bins);
            if (b >= 0) atomicAdd(&hist_s[i * bins + b], 1u);
          }
        }
      }
    }
    keys[e] = key;
  }

  // 2. moments: lanes, then waves
  if (a.moments) {
    for (int i = 0; i < IRRL_EVAL_ENSEMBLE_DIM; i++) {
      const double s1 = ens_wave_sum(sx[i]), s2 = ens_wave_sum(sxx[i]);
      if (lane == 0) { sum_s[wave][2 * i] = s1; sum_s[wave][2 * i + 1] = s2; }
    }
  }
  __syncthreads();
  if (a.moments && tid < 2 * IRRL_EVAL_ENSEMBLE_DIM) {
    double s = 0.0;
    for (int w = 0; w < ENS_WAVES; w++) s += sum_s[w][tid];
    a.moments[cell * (2 * IRRL_EVAL_ENSEMBLE_DIM) + (size_t)tid] = s;
  }
  if (bins > 0)
    for (int i = tid; i < IRRL_EVAL_ENSEMBLE_DIM * bins; i += ENS_THREADS) a.hist[cell * (size_t)(IRRL_EVAL_ENSEMBLE_DIM * bins) + (size_t)i] = hist_s[i];

  // 3. bitonic sort, ascending (the barrier above ordered the keys' stores)
  const int half = P >> 1;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < half; i += ENS_THREADS) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const uint64_t u = keys[lo], v = keys[hi];
        if ((u > v) == up) { keys[lo] = v; keys[hi] = u; }
      }
      __syncthreads();
    }
  }

  // M = the number of kept keys: one position at most is the last non-sentinel
  for (int i = tid; i < P; i += ENS_THREADS)
    if (keys[i] != ENS_SENTINEL && (i == P - 1 || keys[i + 1] == ENS_SENTINEL)) kept_s = (unsigned int)(i + 1);
  __syncthreads();
  const unsigned int M = kept_s;

  // 4. + 5. runs
  double h = 0.0;
  unsigned int occupied = 0u, largest = 0u;
  int carry = -1;                                           // the last run start in front of this round
  const int rounds = (P + ENS_THREADS - 1) / ENS_THREADS;
  for (int r = 0; r < rounds; r++) {
    const int i = r * ENS_THREADS + tid;
    const bool in = i < P;
    const uint64_t key = in ? keys[i] : ENS_SENTINEL;
    const bool live = key != ENS_SENTINEL;
    const bool start = live && (i == 0 || keys[i - 1] != key);
    const bool end = live && (i == P - 1 || keys[i + 1] != key);
    int v = start ? i : -1;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(v, d, 64);
      if (lane >= d) v = o > v ? o : v;
    }
    int *buf = scan_s[r & 1];
    if (lane == 63) buf[wave] = v;
    __syncthreads();
    int first = carry, all = carry;
    for (int w = 0; w < ENS_WAVES; w++) {
      const int t = buf[w];
      if (w < wave) first = t > first ? t : first;
      all = t > all ? t : all;
    }
    if (end) {
      const int s = v > first ? v : first;
      const unsigned int n = (unsigned int)(i - s + 1);
      const double p = (double)n / (double)M;
      const double term = p * log(p);
      h -= term;
      occupied += 1u;
      largest = n > largest ? n : largest;
    }
    carry = all;
  }
  h = ens_wave_sum(h);
  for (int d = 32; d > 0; d >>= 1) {
    occupied += __shfl_xor(occupied, d, 64);
    const unsigned int o = __shfl_xor(largest, d, 64);
    largest = o > largest ? o : largest;
  }
  if (lane == 0) { h_s[wave] = h; runs_s[wave][0] = occupied; runs_s[wave][1] = largest; }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    unsigned int occ = 0u, big = 0u;
    for (int w = 0; w < ENS_WAVES; w++) {
      total += h_s[w];
      occ += runs_s[w][0];
      big = runs_s[w][1] > big ? runs_s[w][1] : big;
    }
    a.entropy[cell] = total;
    if (a.counts) { a.counts[cell * 3] = M; a.counts[cell * 3 + 1] = occ; a.counts[cell * 3 + 2] = big; }
  }
}

hipError_t irrl_eval_ensemble_launch(const EnsembleArgs &a, hipStream_t stream) {
  const size_t lds = (size_t)a.P * sizeof(uint64_t);
  if (lds > 65536) {      // more dynamic LDS than a kernel gets by default: 128 KB for the largest ensemble, of the CU's 160 KB
    const hipError_t e = hipFuncSetAttribute((const void *)irrl_eval_ensemble_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(irrl_eval_ensemble_kernel, dim3((unsigned)a.F, (unsigned)a.C), dim3(ENS_THREADS), lds, stream, a);
  return hipGetLastError();
}
