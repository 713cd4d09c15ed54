// eval_spectrum.hip -- the spectrogram and the Welch spectrum of recorder columns (irrl_eval_spectrum, include/irrl_env.h): per robot the
// one-sided power spectral density of every segment of nperseg frames, hop frames apart, that lies inside the robot's frames i < T_e; their
// sum per condition; and the segments themselves for up to 8 chosen robots.  A translation unit of its own, compiled by the plain driver; no
// global atomics and no floating-point atomics: every output word has exactly one writer and ONE order of additions, whatever the grid
// (csrc/eval_elements.hpp irrl_eval_spectrum_*: per bin the samples of a segment in ascending order, per robot the segments in ascending order,
// per condition the robots in ascending order).
//
// WHY A DIRECT DFT.  An FFT's error depends on its factorisation, and v_mfma_f64_16x16x4_f64 adds in an order the ISA does not state.  A dot
// product of length n errs by at most n 2^-53 sum |a_n t_n| in ANY order, fused or not, which gives the tests a bound that is derived and not
// measured; and nperseg need not be a power of two.  The price is nperseg / log2(nperseg) times the multiply-adds, on a unit that has f64 to
// spare next to what the evaluation loop itself costs.  Do not "optimise" this into an FFT or into MFMA without a new bound.
//
// WHY THE ZERO IS AN ARGUMENT: as in eval_correlation.hip (-fno-signed-zeros lets the compiler fold 0.0 + p to p).
//
// irrl_eval_spectrum_kernel, one workgroup per (robot, block of SP_CB = 4 columns), thread = frequency bin k (as many waves as the K = nperseg /
// 2 + 1 bins need, at most 256 threads, looped over the bins beyond).  LDS, all of it dynamic and 16-byte aligned: the twiddles tw [nperseg][2]
// (16 KB at nperseg = 1024), the segment a [nperseg][4] (32 KB), the window [nperseg] (8 KB), the four means, T_e.
//   1. T_e: the first analysed frame with a non-zero rec_done word, an integer LDS atomicMin (a minimum has no order); S_e from it.  Thread 0
//      adds the window's squares in order for the density (the window is a device table: the host never reads it).
//   2. per segment: its 4 columns are loaded, scaled and stored as f64; with a detrend thread c < 4 adds column c in ascending order and divides;
//      every word becomes a_n = (v_n - m) window[n] in place.
//   3. thread k walks n = 0 .. nperseg - 1: a_n of the 4 columns is two 16-byte LDS reads every lane shares (a broadcast), the twiddle one 16-byte
//      gather at (k n) mod nperseg, kept as a running index; 8 f64 multiply-adds per 3 reads.  P_k goes to `sxx` where the robot is listed and
//      into the thread's running sum, a register across the robot's segments.
//   4. the running sums are stored once: to psd_sum with one robot per condition, to the robot's partials in `work` otherwise.
// irrl_eval_spectrum_sum_kernel (robots > 1), one thread per (condition, word): the robots' partials in ascending order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eval_spectrum.hpp"

#define SP_THREADS 256
#define SP_CB IRRL_EVAL_SPECTRUM_CB

// the doubles of dynamic LDS: tw | segment | window | means | T_e (one more double's room)
static inline size_t spectrum_lds_doubles(int nperseg) { return (size_t)nperseg * (size_t)(3 + SP_CB) + SP_CB + 2; }

__global__ __launch_bounds__(SP_THREADS) void irrl_eval_spectrum_kernel(const SpectrumArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sp_lds[];
  const int P = a.spec.nperseg, K = a.K, hop = a.spec.hop, detrend = a.spec.detrend;
  double2 *tw_s = reinterpret_cast<double2 *>(sp_lds);                  // [P]: cos, sin
  double *seg = sp_lds + 2 * (size_t)P;                                 // [P][SP_CB], byte offset 16 P
  const double2 *seg2 = reinterpret_cast<const double2 *>(seg);
  double *win_s = seg + (size_t)SP_CB * (size_t)P;                      // [P]
  double *mean_s = win_s + P;                                           // [SP_CB]
  double *dens_s = mean_s + SP_CB;                                      // [1]
  int *te_s = reinterpret_cast<int *>(dens_s + 1);
  const int e = (int)blockIdx.x, c0 = (int)blockIdx.y * SP_CB, tid = (int)threadIdx.x, threads = (int)blockDim.x;
  const int T = a.T, N = a.N, cx = a.spec.x_count;

  if (tid == 0) *te_s = T;
  for (int n = tid; n < P; n += threads) {
    tw_s[n] = make_double2(a.tw[2 * n], a.tw[2 * n + 1]);
    win_s[n] = a.window[n];
  }
  __syncthreads();
  if (a.rec_done)
    for (int i = tid; i < T; i += threads) {
      const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i);
      if (a.rec_done[row * (size_t)N + (size_t)e] != 0) atomicMin(te_s, i);
    }
  if (tid == 0) *dens_s = irrl_eval_spectrum_density(win_s, P, a.spec.fs, a.zero);
  __syncthreads();
  const int Se = irrl_eval_spectrum_segments(*te_s, P, hop);
  const double density = *dens_s;

  const size_t xrow = (size_t)N * (size_t)a.spec.x_dim;
  const float *xe = a.x + (size_t)e * (size_t)a.spec.x_dim + (size_t)a.spec.x_first + (size_t)c0;
  double *out = a.p_psd + ((size_t)e * (size_t)cx + (size_t)c0) * (size_t)K;
  const size_t S_max = (size_t)a.S_max;

  for (int k0 = 0; k0 < K; k0 += threads) {
    const int k = k0 + tid;
    const bool live = k < K;
    const double gain = irrl_eval_spectrum_gain(k, P);
    double psd[SP_CB];
#pragma unroll
    for (int c = 0; c < SP_CB; c++) psd[c] = a.zero;
    for (int s = 0; s < Se; s++) {                              // (Se is the workgroup's: every thread meets every barrier)
      __syncthreads();                                          // the last segment's words have been read
      for (int q = tid; q < SP_CB * P; q += threads) {
        const int n = q / SP_CB, c = q % SP_CB;
        double v = 0.0;                                         // (a column beyond cx: its bins are never stored)
        if (c0 + c < cx) {
          const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, s * hop + n);
          v = irrl_eval_spectrum_sample(xe[row * xrow + (size_t)c], a.spec.scale[c0 + c]);
        }
        seg[q] = v;
      }
      __syncthreads();
      if (detrend) {
        if (tid < SP_CB) mean_s[tid] = irrl_eval_spectrum_mean(seg + tid, SP_CB, P, a.zero);
        __syncthreads();
      }
      for (int q = tid; q < SP_CB * P; q += threads)
        seg[q] = irrl_eval_spectrum_windowed(seg[q], detrend ? mean_s[q % SP_CB] : 0.0, detrend, win_s[q / SP_CB]);
      __syncthreads();
      if (live) {
        double re[SP_CB], si[SP_CB];
#pragma unroll
        for (int c = 0; c < SP_CB; c++) { re[c] = a.zero; si[c] = a.zero; }
        int j = 0;
        for (int n = 0; n < P; n++) {
          const double2 t = tw_s[j];
          const double2 a01 = seg2[2 * n], a23 = seg2[2 * n + 1];
          const double an[SP_CB] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
          for (int c = 0; c < SP_CB; c++) {
            re[c] = irrl_eval_spectrum_add(re[c], an[c], t.x);
            si[c] = irrl_eval_spectrum_add(si[c], an[c], t.y);
          }
          j = irrl_eval_spectrum_step(j, k, P);
        }
#pragma unroll
        for (int c = 0; c < SP_CB; c++) {
          const double p = irrl_eval_spectrum_power(re[c], si[c], gain, density);
          psd[c] = psd[c] + p;
          if (a.sxx && c0 + c < cx)
            for (int m = 0; m < a.spec.matrix_count; m++)
              if (a.spec.matrix_env[m] == e) a.sxx[(((size_t)m * (size_t)cx + (size_t)(c0 + c)) * S_max + (size_t)s) * (size_t)K + (size_t)k] = p;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < SP_CB; c++)
        if (c0 + c < cx) {
          out[(size_t)c * (size_t)K + (size_t)k] = psd[c];
          if (a.sxx)
            for (int m = 0; m < a.spec.matrix_count; m++)
              if (a.spec.matrix_env[m] == e)
                for (size_t s = (size_t)Se; s < S_max; s++)       // the segments the robot did not live to see
                  a.sxx[(((size_t)m * (size_t)cx + (size_t)(c0 + c)) * S_max + s) * (size_t)K + (size_t)k] = 0.0;
        }
    }
  }
  if (blockIdx.y == 0 && tid == 0) a.p_seg[e] = (int64_t)Se;
}

// one thread per (condition, word): the cx K sums | the segment count; the robots' partials in ascending robot order
__global__ __launch_bounds__(SP_THREADS) void irrl_eval_spectrum_sum_kernel(const SpectrumArgs a) {
  const size_t sums = (size_t)a.spec.x_count * (size_t)a.K, per = sums + 1;
  const size_t idx = (size_t)blockIdx.x * SP_THREADS + (size_t)threadIdx.x;
  if (idx >= (size_t)a.C * per) return;
  const size_t g = idx / per, q = idx % per, env0 = g * (size_t)a.R;
  const int R = a.R;
  if (q < sums) {
    const double *src = a.p_psd + env0 * sums + q;
    double t = a.zero;
    for (int r = 0; r < R; r++) t = t + src[(size_t)r * sums];
    a.psd_sum[g * sums + q] = t;
  } else {
    int64_t t = 0;
    for (int r = 0; r < R; r++) t += a.p_seg[env0 + (size_t)r];
    a.segments[g] = t;
  }
}

hipError_t irrl_eval_spectrum_launch(const SpectrumArgs &a, hipStream_t stream) {
  const int waves = (a.K + 63) / 64, blocks_y = (a.spec.x_count + SP_CB - 1) / SP_CB;
  const size_t lds = spectrum_lds_doubles(a.spec.nperseg) * sizeof(double);
  hipLaunchKernelGGL(irrl_eval_spectrum_kernel, dim3((unsigned)a.N, (unsigned)blocks_y), dim3(waves > 4 ? SP_THREADS : 64u * (unsigned)waves), lds, stream,
                     a);
  if (a.R > 1) {
    const size_t words = (size_t)a.C * ((size_t)a.spec.x_count * (size_t)a.K + 1), blocks = (words + SP_THREADS - 1) / SP_THREADS;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(irrl_eval_spectrum_sum_kernel, dim3((unsigned)blocks), dim3(SP_THREADS), 0, stream, a);
  }
  return hipGetLastError();
}
