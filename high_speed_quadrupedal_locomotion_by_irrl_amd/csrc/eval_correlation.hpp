// eval_correlation.hpp -- what the C-ABI (irrl_env_abi.hip: irrl_eval_correlation, which checks the arguments) and the kernels' translation
// unit (eval_correlation.hip) share: the kernels' argument block and their launcher.
#pragma once
#include <hip/hip_runtime.h>
#include "eval_elements.hpp"

struct CorrelationArgs {
  const float *x, *y;          // [rows, N, x_dim], [rows, N, y_dim]
  const uint8_t *rec_done;     // [rows, N] or NULL
  int N, C, R, T;              // pool size, conditions, robots per condition (N = C R), analysed frames (1 .. IRRL_EVAL_CORR_MAX_FRAMES)
  int frame_first, frame_every;
  irrl_eval_corr_spec spec;
  double zero;                 // +0.0, the start of every accumulator (why it travels as an argument: eval_correlation.hip)
  // what the first kernel writes per robot e -- the outputs themselves with R == 1, the regions of `work` otherwise
  double *p_sxy, *p_sx, *p_sy; // [N, cx, cy], [N, cx, 2], [N, cy, 2]
  int64_t *p_count;            // [N]: T_e
  float *p_rx, *p_ry;          // [N, cx, 2], [N, cy, 2]; both NULL: ranges off
  // what the second kernel (R > 1 only) writes per condition
  double *sxy, *sx, *sy;
  int64_t *count;
  float *range_x, *range_y;    // both NULL: off
};

// the regions of `work` (R > 1): f64 sxy [N, cx cy] | f64 sx [N, 2 cx] | f64 sy [N, 2 cy] | i64 T_e [N] | f32 range_x [N, 2 cx] | f32 range_y [N, 2 cy]
static inline void irrl_eval_corr_work_regions(CorrelationArgs &a, double *work) {
  const size_t N = (size_t)a.N, cx = (size_t)a.spec.x_count, cy = (size_t)a.spec.y_count;
  a.p_sxy = work;
  a.p_sx = a.p_sxy + N * cx * cy;
  a.p_sy = a.p_sx + N * 2 * cx;
  a.p_count = reinterpret_cast<int64_t *>(a.p_sy + N * 2 * cy);
  a.p_rx = reinterpret_cast<float *>(a.p_count + N);
  a.p_ry = a.p_rx + N * 2 * cx;
}

// one launch over N workgroups and, with R > 1, a second over the conditions' accumulators, on `stream`; the arguments have been checked
hipError_t irrl_eval_correlation_launch(const CorrelationArgs &a, hipStream_t stream);
