// eval_correlation.hip -- the correlation moments of two recorder windows (irrl_eval_correlation, include/irrl_env.h): count, sum x, sum x^2,
// sum y, sum y^2, sum x y and the ranges per condition.  A translation unit of its own, compiled by the plain driver; no global atomics and no
// floating-point atomics: every output word has exactly one writer and ONE order of additions, whatever the grid (csrc/eval_elements.hpp
// irrl_eval_corr_add: per robot the frames in ascending order, per condition the robots in ascending order).
//
// WHY NOT THE MATRIX CORES.  sum x y is a [cx, T] x [T, cy] product and v_mfma_f64_16x16x4_f64 would do it, but the instruction adds its four
// products and C in an order the ISA does not state, and a numpy twin cannot follow an order nobody wrote down.  The kernel is bound by reading
// the recorder (4 cy bytes per frame against 2 cx cy flops on a unit that has them to spare), so the matrix cores would buy nothing and cost the
// bit-for-bit test against the twin and the host program.  Do not "optimise" this into MFMA.
//
// WHY THE ZERO IS AN ARGUMENT.  The library is compiled with -fno-signed-zeros, under which the compiler may fold 0.0 + p to p.  p = -0.0 happens
// (a zero sample times a negative one) and would then survive as -0.0 where IEEE, the host program and numpy give +0.0 + -0.0 = +0.0.  An
// accumulator that starts from a value the compiler cannot see is added to in earnest; CorrelationArgs::zero is +0.0.
//
// irrl_eval_correlation_kernel, one workgroup per robot, thread = y column: as many waves as the y window has columns, at most 256 threads (looped
// over the columns beyond; a 35-column window is one wave, so that a CU holds four times the robots):
//   1. T_e: the first analysed frame with a non-zero rec_done word, an integer LDS atomicMin (a minimum has no order).
//   2. for every tile of CR_XT = 8 x columns one serial pass over the frames i < T_e: the tile's x words of CR_CHUNK = 64 frames are staged in
//      LDS (they are wave-uniform: every thread reads the same word, a broadcast), a frame's y window is one coalesced row of 4 cy bytes, loaded
//      CR_FB = 8 frames ahead of its use, and each thread adds into its 8 f64 accumulators.  sum y, sum y^2, min and max ride along in the first
//      tile's pass only; the x-only sums of column c0 + t go to thread t < 8 of the first y block, out of the staged words.
//   3. every accumulator is stored once: to the outputs with one robot per condition, to the robot's partials in `work` otherwise.
// irrl_eval_correlation_sum_kernel (robots > 1), one thread per (condition, accumulator): the robots' partials in ascending order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "eval_correlation.hpp"

#define CR_THREADS 256
#define CR_XT 8
#define CR_CHUNK 64
#define CR_FB 8

__global__ __launch_bounds__(CR_THREADS) void irrl_eval_correlation_kernel(const CorrelationArgs a) {
  __shared__ float xs[CR_CHUNK * CR_XT];
  __shared__ int te_s;
  const int e = (int)blockIdx.x, tid = (int)threadIdx.x, threads = (int)blockDim.x;
  const int T = a.T, N = a.N, cx = a.spec.x_count, cy = a.spec.y_count;

  if (tid == 0) te_s = T;
  __syncthreads();
  if (a.rec_done)
    for (int i = tid; i < T; i += threads) {
      const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i);
      if (a.rec_done[row * (size_t)N + (size_t)e] != 0) atomicMin(&te_s, i);
    }
  __syncthreads();
  const int Te = te_s;

  const size_t xrow = (size_t)N * (size_t)a.spec.x_dim, yrow = (size_t)N * (size_t)a.spec.y_dim;
  const float *xe = a.x + (size_t)e * (size_t)a.spec.x_dim + (size_t)a.spec.x_first;
  const float *ye = a.y + (size_t)e * (size_t)a.spec.y_dim + (size_t)a.spec.y_first;
  double *o_sxy = a.p_sxy + (size_t)e * (size_t)cx * (size_t)cy, *o_sx = a.p_sx + (size_t)e * 2 * (size_t)cx, *o_sy = a.p_sy + (size_t)e * 2 * (size_t)cy;
  const bool ranges = a.p_rx != nullptr && a.p_ry != nullptr;

  for (int j0 = 0; j0 < cy; j0 += threads) {
    const int j = j0 + tid;
    const bool live = j < cy;
    for (int c0 = 0; c0 < cx; c0 += CR_XT) {
      const bool first = c0 == 0;                               // the pass that takes the y-only sums of its columns along
      const bool xown = j0 == 0 && tid < CR_XT && c0 + tid < cx;   // this thread takes the x-only sums of column c0 + tid
      double acc[CR_XT];
#pragma unroll
      for (int k = 0; k < CR_XT; k++) acc[k] = a.zero;
      double y1 = a.zero, y2 = a.zero, x1 = a.zero, x2 = a.zero;
      float ylo = INFINITY, yhi = -INFINITY, xlo = INFINITY, xhi = -INFINITY;
      for (int i0 = 0; i0 < Te; i0 += CR_CHUNK) {               // (Te is the workgroup's: every thread meets every barrier)
        const int nf = Te - i0 < CR_CHUNK ? Te - i0 : CR_CHUNK;
        __syncthreads();                                        // the last chunk's words have been read
        for (int q = tid; q < CR_CHUNK * CR_XT; q += threads) {
          const int f = q / CR_XT, k = q % CR_XT;
          float v = 0.0f;                                       // (a column beyond cx: its accumulator is never stored)
          if (f < nf && c0 + k < cx) v = xe[(size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i0 + f) * xrow + (size_t)(c0 + k)];
          xs[q] = v;
        }
        __syncthreads();
        if (xown)
          for (int f = 0; f < nf; f++) {
            const float v = xs[f * CR_XT + tid];
            x1 = irrl_eval_corr_add(x1, v, 1.0f);
            x2 = irrl_eval_corr_add(x2, v, v);
            xlo = irrl_eval_corr_min(xlo, v);
            xhi = irrl_eval_corr_max(xhi, v);
          }
        if (live)
          for (int f0 = 0; f0 < nf; f0 += CR_FB) {
            float yv[CR_FB];
#pragma unroll
            for (int u = 0; u < CR_FB; u++)
              yv[u] = f0 + u < nf ? ye[(size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i0 + f0 + u) * yrow + (size_t)j] : 0.0f;
#pragma unroll
            for (int u = 0; u < CR_FB; u++) {
              if (f0 + u >= nf) break;
              const float *xf = xs + (f0 + u) * CR_XT;
#pragma unroll
              for (int k = 0; k < CR_XT; k++) acc[k] = irrl_eval_corr_add(acc[k], xf[k], yv[u]);
              if (first) {
                y1 = irrl_eval_corr_add(y1, yv[u], 1.0f);
                y2 = irrl_eval_corr_add(y2, yv[u], yv[u]);
                ylo = irrl_eval_corr_min(ylo, yv[u]);
                yhi = irrl_eval_corr_max(yhi, yv[u]);
              }
            }
          }
      }
      if (live) {
#pragma unroll
        for (int k = 0; k < CR_XT; k++)
          if (c0 + k < cx) o_sxy[(size_t)(c0 + k) * (size_t)cy + (size_t)j] = acc[k];
        if (first) {
          o_sy[2 * j] = y1; o_sy[2 * j + 1] = y2;
          if (ranges) {
            float *o_ry = a.p_ry + (size_t)e * 2 * (size_t)cy;
            o_ry[2 * j] = ylo; o_ry[2 * j + 1] = yhi;
          }
        }
      }
      if (xown) {
        o_sx[2 * (c0 + tid)] = x1; o_sx[2 * (c0 + tid) + 1] = x2;
        if (ranges) {
          float *o_rx = a.p_rx + (size_t)e * 2 * (size_t)cx;
          o_rx[2 * (c0 + tid)] = xlo; o_rx[2 * (c0 + tid) + 1] = xhi;
        }
      }
    }
  }
  if (tid == 0) a.p_count[e] = (int64_t)Te;
}

// one thread per (condition, word): the sums | the count | the ranges; the robots' partials in ascending robot order
__global__ __launch_bounds__(CR_THREADS) void irrl_eval_correlation_sum_kernel(const CorrelationArgs a) {
  const size_t cx = (size_t)a.spec.x_count, cy = (size_t)a.spec.y_count, nxy = cx * cy, sums = nxy + 2 * cx + 2 * cy;
  const size_t per = sums + 1 + 2 * cx + 2 * cy;
  const size_t idx = (size_t)blockIdx.x * CR_THREADS + (size_t)threadIdx.x;
  if (idx >= (size_t)a.C * per) return;
  const size_t g = idx / per, q = idx % per, env0 = g * (size_t)a.R;
  const int R = a.R;
  if (q < sums) {
    const double *src;
    double *dst;
    size_t stride;
    if (q < nxy) { stride = nxy; src = a.p_sxy + env0 * stride + q; dst = a.sxy + g * stride + q; }
    else if (q < nxy + 2 * cx) { stride = 2 * cx; src = a.p_sx + env0 * stride + (q - nxy); dst = a.sx + g * stride + (q - nxy); }
    else { stride = 2 * cy; src = a.p_sy + env0 * stride + (q - nxy - 2 * cx); dst = a.sy + g * stride + (q - nxy - 2 * cx); }
    double t = a.zero;
    for (int r = 0; r < R; r++) t = t + src[(size_t)r * stride];
    *dst = t;
  } else if (q == sums) {
    int64_t t = 0;
    for (int r = 0; r < R; r++) t += a.p_count[env0 + (size_t)r];
    a.count[g] = t;
  } else if (a.range_x != nullptr && a.range_y != nullptr) {
    size_t k = q - sums - 1;
    const float *src;
    float *dst;
    size_t stride;
    if (k < 2 * cx) { stride = 2 * cx; src = a.p_rx + env0 * stride + k; dst = a.range_x + g * stride + k; }
    else { k -= 2 * cx; stride = 2 * cy; src = a.p_ry + env0 * stride + k; dst = a.range_y + g * stride + k; }
    const bool is_max = (k & 1) != 0;
    float m = is_max ? -INFINITY : INFINITY;
    for (int r = 0; r < R; r++) {
      const float v = src[(size_t)r * stride];
      m = is_max ? irrl_eval_corr_max(m, v) : irrl_eval_corr_min(m, v);
    }
    *dst = m;
  }
}

hipError_t irrl_eval_correlation_launch(const CorrelationArgs &a, hipStream_t stream) {
  const int waves = (a.spec.y_count + 63) / 64;
  hipLaunchKernelGGL(irrl_eval_correlation_kernel, dim3((unsigned)a.N), dim3(waves > 4 ? CR_THREADS : 64u * (unsigned)waves), 0, stream, a);
  if (a.R > 1) {
    const size_t cx = (size_t)a.spec.x_count, cy = (size_t)a.spec.y_count;
    const size_t words = (size_t)a.C * (cx * cy + 4 * cx + 4 * cy + 1), blocks = (words + CR_THREADS - 1) / CR_THREADS;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(irrl_eval_correlation_sum_kernel, dim3((unsigned)blocks), dim3(CR_THREADS), 0, stream, a);
  }
  return hipGetLastError();
}
