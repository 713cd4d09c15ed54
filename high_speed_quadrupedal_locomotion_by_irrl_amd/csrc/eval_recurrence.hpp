// eval_recurrence.hpp -- what the C-ABI (irrl_env_abi.hip: irrl_eval_recurrence, which checks the arguments) and the kernel's translation unit
// (eval_recurrence.hip) share: the kernel's argument block and its launcher.
#pragma once
#include <hip/hip_runtime.h>
#include "eval_elements.hpp"

struct RecurrenceArgs {
  const float *rec_body;       // [rows, N, 13]
  int N, T;                    // pool size = the grid; analysed frames per robot (1 .. IRRL_EVAL_RECURRENCE_MAX_FRAMES)
  int frame_first, frame_every;
  irrl_eval_recurrence_spec spec;
  double threshold;            // irrl_eval_recurrence_threshold(eps, steps, radius): R_ij <=> d2 < threshold
  uint32_t *counts;            // [N, 9]
  uint32_t *lag;               // [N, spec.lags] or NULL
  uint8_t *matrix;             // [spec.matrix_count, T, T] or NULL
};

// the workgroup's dynamic LDS: the states [6][T] f64 and a kept byte per frame
static inline size_t irrl_eval_recurrence_lds(int T) {
  return (size_t)IRRL_EVAL_ENSEMBLE_DIM * (size_t)T * sizeof(double) + (((size_t)T + 15) & ~(size_t)15);
}

// one launch of irrl_eval_recurrence_kernel over N workgroups on `stream`; the arguments have been checked (N >= 1, T >= 1)
hipError_t irrl_eval_recurrence_launch(const RecurrenceArgs &a, hipStream_t stream);
