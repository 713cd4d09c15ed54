// eval_spectrum.hpp -- what the C-ABI (irrl_env_abi.hip: irrl_eval_spectrum, which checks the arguments) and the kernels' translation unit
// (eval_spectrum.hip) share: the kernels' argument block and their launcher.
#pragma once
#include <hip/hip_runtime.h>
#include "eval_elements.hpp"

#define IRRL_EVAL_SPECTRUM_CB 4   // the columns one workgroup analyses

// (the spec's scale[64] and matrix_env[8] travel in the argument block: 640 of the 4096 bytes a kernel's arguments may take)
struct SpectrumArgs {
  const float *x;              // [rows, N, x_dim]
  const uint8_t *rec_done;     // [rows, N] or NULL
  const double *window, *tw;   // [nperseg], [nperseg, 2]
  int N, C, R, T;              // pool size, conditions, robots per condition (N = C R), analysed frames (nperseg .. IRRL_EVAL_SPECTRUM_MAX_FRAMES)
  int frame_first, frame_every;
  int K, S_max;                // nperseg / 2 + 1, (T - nperseg) / hop + 1
  irrl_eval_spectrum_spec spec;
  double zero;                // +0.0, the start of every accumulator (why it travels as an argument: eval_correlation.hip)
  // what the first kernel writes per robot e -- the outputs themselves with R == 1, the regions of `work` otherwise
  double *p_psd;               // [N, cx, K]
  int64_t *p_seg;              // [N]: S_e
  double *sxx;                 // [matrix_count, cx, S_max, K] or NULL
  // what the second kernel (R > 1 only) writes per condition
  double *psd_sum;             // [C, cx, K]
  int64_t *segments;           // [C]
};

// the regions of `work` (R > 1): f64 partials [N, cx K] | i64 S_e [N]
static inline void irrl_eval_spectrum_work_regions(SpectrumArgs &a, double *work) {
  a.p_psd = work;
  a.p_seg = reinterpret_cast<int64_t *>(work + (size_t)a.N * (size_t)a.spec.x_count * (size_t)a.K);
}

// one launch over N x ceil(cx / 4) workgroups and, with R > 1, a second over the conditions' words, on `stream`; the arguments have been checked
hipError_t irrl_eval_spectrum_launch(const SpectrumArgs &a, hipStream_t stream);
