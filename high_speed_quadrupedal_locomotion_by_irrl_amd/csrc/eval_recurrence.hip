// eval_recurrence.hip -- the recurrence analysis of a body recorder (irrl_eval_recurrence, include/irrl_env.h): one workgroup per robot turns
// the robot's T recorder rows into normalised states in LDS (csrc/eval_elements.hpp), walks the time x time matrix of their distances along its
// diagonals and along its columns with run-length counters and reduces integer counts.  A translation unit of its own, compiled by the plain
// driver; no global atomics and no floating-point atomics: every output word has exactly one writer.
//
// Order of the work in a workgroup of 512 threads (8 waves):
//   1. states: thread t takes frames t, t + 512, ...: features, u = (x - mid) / width into dynamic LDS as [6][T] f64 (structure of arrays) and
//      a kept byte per frame.  Zeros stand in for a dropped frame's state; the kept byte decides.
//   2. diagonals: thread t owns lag tau = 1 + t, 1 + t + 512, ... <= T / 2 TOGETHER with lag T - tau: T - tau pairs (s, s + tau) and then tau
//      pairs (s - (T - tau), s), T steps whatever tau is, so every lane of a wave runs the same trip count.  With consecutive lanes on consecutive
//      lags, u[k][s + tau] are consecutive 8-byte words (a half-wave's ds_read_b64 touch all 64 banks once) and u[k][s] is one word for the wave,
//      a broadcast; an array-of-structures row of 12 dwords would put lanes 16 apart on the same bank.  Per lag: a run-length counter closes a
//      line at a non-recurrent point and at the matrix border, the lag's own recurrence count goes to lag[e, l] (one writer), and lags >= w add
//      to REC, DIAG_POINTS, DIAG_LINES, DIAG_MAX.  R_ij is decided as d2 < threshold (the smallest d2 whose level reaches the radius, found on
//      the host from the level function itself: no square root, no division).  A robot listed in matrix_env takes the level function instead and
//      stores q at [i, j] (consecutive bytes over the lanes) and at [j, i] (strided: at most 8 robots of a call pay for it).
//   3. columns: thread t owns column j = t, t + 512, ... with u_j in registers and walks i = 0 .. T - 1 (u[k][i]: a broadcast) through the full
//      matrix with the band |i - j| < w removed: VERT_POINTS, VERT_LINES, VERT_MAX, REC_FULL.  By symmetry column j is row j.
//   4. the nine counters: xor-butterfly over the 64 lanes of a wave (sums, two maxima), the 8 waves through LDS, one thread per counter.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eval_recurrence.hpp"

#define REC_THREADS 512
#define REC_WAVES (REC_THREADS / 64)

// a line of `run` points ends: longest line of any length, and points / lines of those that reach `least`
static __device__ __forceinline__ void rec_close(unsigned run, unsigned least, unsigned &points, unsigned &lines, unsigned &longest) {
  if (run == 0u) return;
  if (run >= least) { points += run; lines += 1u; }
  longest = run > longest ? run : longest;
}

__global__ __launch_bounds__(REC_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void irrl_eval_recurrence_kernel(const RecurrenceArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rec_lds[];
  __shared__ unsigned int part_s[REC_WAVES][IRRL_EVAL_RECURRENCE_COUNTS];
  const int T = a.T;
  double *u = reinterpret_cast<double *>(rec_lds);                                        // [6][T]
  uint8_t *kept = rec_lds + (size_t)IRRL_EVAL_ENSEMBLE_DIM * (size_t)T * sizeof(double);   // [T]

  const int e = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int steps = a.spec.steps, radius = a.spec.radius;
  const int W = a.spec.theiler > 1 ? a.spec.theiler : 1;
  const int lags = a.lag ? a.spec.lags : 0;
  const double eps = a.spec.eps, thr = a.threshold;
  unsigned slots = 0u;                                      // the matrices this robot fills
  if (a.matrix)
    for (int s = 0; s < a.spec.matrix_count; s++)
      if (a.spec.matrix_env[s] == e) slots |= 1u << s;
  const size_t TT = (size_t)T * (size_t)T;

  // 1. states
  unsigned n_kept = 0u;
  for (int i = tid; i < T; i += REC_THREADS) {
    const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i);
    double x[IRRL_EVAL_ENSEMBLE_DIM];
    irrl_eval_ensemble_features(a.rec_body + (row * (size_t)a.N + (size_t)e) * 13, x);
    const bool ok = irrl_eval_recurrence_state(x, a.spec, u + i, (size_t)T);
    if (!ok)
      for (int k = 0; k < IRRL_EVAL_ENSEMBLE_DIM; k++) u[(size_t)k * (size_t)T + (size_t)i] = 0.0;
    kept[i] = ok ? 1 : 0;
    n_kept += ok ? 1u : 0u;
    for (unsigned m = slots; m != 0u; m &= m - 1u) {        // the main diagonal: d = 0 for a kept frame
      const size_t s = (size_t)(__ffs(m) - 1);
      a.matrix[s * TT + (size_t)i * (size_t)T + (size_t)i] = (uint8_t)(ok ? 0 : steps);
    }
  }
  __syncthreads();

  // 2. diagonals
  unsigned rec = 0u, dpoints = 0u, dlines = 0u, dmax = 0u;
  const unsigned lmin = (unsigned)a.spec.lmin, vmin = (unsigned)a.spec.vmin;
  const int half = T >> 1;
  for (int tau = 1 + tid; tau <= half; tau += REC_THREADS) {
    const int nA = T - tau;                                 // pairs of lag tau; lag T - tau = nA has tau pairs
    const bool hasB = nA != tau;
    unsigned run = 0u, cnt = 0u;
    for (int s = 0; s < T; s++) {
      if (s == nA) {                                        // the border of lag tau: close, hand out, go on with lag nA
        if (tau >= W) { rec_close(run, lmin, dpoints, dlines, dmax); rec += cnt; }
        if (tau < lags) a.lag[(size_t)e * (size_t)lags + (size_t)tau] = cnt;
        run = 0u; cnt = 0u;
        if (!hasB) break;
      }
      const bool inA = s < nA;
      const int i = inA ? s : s - nA, j = inA ? s + tau : s;
      const int l = inA ? tau : nA;
      const bool both = kept[i] != 0 && kept[j] != 0;
      const double d2 = irrl_eval_recurrence_dist2(u + i, (size_t)T, u + j, (size_t)T);
      bool r;
      if (slots != 0u) {
        const int q = both ? irrl_eval_recurrence_level(d2, eps, steps) : steps;
        r = q < radius;
        for (unsigned m = slots; m != 0u; m &= m - 1u) {
          uint8_t *mat = a.matrix + (size_t)(__ffs(m) - 1) * TT;
          mat[(size_t)i * (size_t)T + (size_t)j] = (uint8_t)q;
          mat[(size_t)j * (size_t)T + (size_t)i] = (uint8_t)q;
        }
      } else {
        r = both && d2 < thr;
      }
      if (r) { run += 1u; cnt += 1u; }
      else {
        if (l >= W) rec_close(run, lmin, dpoints, dlines, dmax);
        run = 0u;
      }
    }
    if (hasB) {                                             // the border of lag nA
      if (nA >= W) { rec_close(run, lmin, dpoints, dlines, dmax); rec += cnt; }
      if (nA < lags) a.lag[(size_t)e * (size_t)lags + (size_t)nA] = cnt;
    }
  }

  // 3. columns
  unsigned vpoints = 0u, vlines = 0u, vmax = 0u, full = 0u;
  for (int j = tid; j < T; j += REC_THREADS) {
    double uj[IRRL_EVAL_ENSEMBLE_DIM];
    for (int k = 0; k < IRRL_EVAL_ENSEMBLE_DIM; k++) uj[k] = u[(size_t)k * (size_t)T + (size_t)j];
    const bool kj = kept[j] != 0;
    unsigned run = 0u;
    for (int i = 0; i < T; i++) {
      const int gap = i > j ? i - j : j - i;
      const double d2 = irrl_eval_recurrence_dist2(u + i, (size_t)T, uj, 1);
      const bool r = gap >= W && kj && kept[i] != 0 && d2 < thr;
      if (r) { run += 1u; full += 1u; }
      else { rec_close(run, vmin, vpoints, vlines, vmax); run = 0u; }
    }
    rec_close(run, vmin, vpoints, vlines, vmax);
  }

  // 4. the counters: lanes, then waves
  unsigned v[IRRL_EVAL_RECURRENCE_COUNTS] = {n_kept, rec, dpoints, dlines, dmax, vpoints, vlines, vmax, full};
  for (int c = 0; c < IRRL_EVAL_RECURRENCE_COUNTS; c++) {
    const bool is_max = c == 4 || c == 7;
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned o = __shfl_xor(v[c], d, 64);
      v[c] = is_max ? (o > v[c] ? o : v[c]) : v[c] + o;
    }
    if (lane == 0) part_s[wave][c] = v[c];
  }
  __syncthreads();
  if (tid < IRRL_EVAL_RECURRENCE_COUNTS) {
    const bool is_max = tid == 4 || tid == 7;
    unsigned t = 0u;
    for (int w = 0; w < REC_WAVES; w++) {
      const unsigned o = part_s[w][tid];
      t = is_max ? (o > t ? o : t) : t + o;
    }
    a.counts[(size_t)e * IRRL_EVAL_RECURRENCE_COUNTS + (size_t)tid] = t;
    if (tid == 0 && lags > 0) a.lag[(size_t)e * (size_t)lags] = t;      // lag 0: the main diagonal, R_ii <=> kept
  }
}

hipError_t irrl_eval_recurrence_launch(const RecurrenceArgs &a, hipStream_t stream) {
  const size_t lds = irrl_eval_recurrence_lds(a.T);
  if (lds > 65536) {      // more dynamic LDS than a kernel gets by default: 98 KB at T = 2048, of the CU's 160 KB
    const hipError_t e = hipFuncSetAttribute((const void *)irrl_eval_recurrence_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(irrl_eval_recurrence_kernel, dim3((unsigned)a.N), dim3(REC_THREADS), lds, stream, a);
  return hipGetLastError();
}
