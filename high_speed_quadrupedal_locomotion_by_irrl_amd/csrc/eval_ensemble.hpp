// eval_ensemble.hpp -- what the C-ABI (irrl_env_abi.hip: irrl_eval_ensemble, which checks the arguments) and the kernel's translation unit
// (eval_ensemble.hip) share: the kernel's argument block and its launcher.
#pragma once
#include <hip/hip_runtime.h>
#include "eval_elements.hpp"

struct EnsembleArgs {
  const float *rec_body;       // [rows, N, 13]
  int N, E;                    // pool size; explorations per condition (1 .. IRRL_EVAL_ENSEMBLE_MAX)
  int P;                       // the next power of two >= E: the length of the sorted array
  int frame_first, frame_every;
  int C, F;                    // the grid: blockIdx.x = analysed frame, blockIdx.y = condition
  const uint8_t *mask;         // [N] or NULL
  irrl_eval_ensemble_spec spec;
  double *entropy;             // [C, F]
  uint32_t *counts;            // [C, F, 3] or NULL
  uint32_t *hist;              // [C, F, 6, hist_bins] or NULL
  double *moments;             // [C, F, 6, 2] or NULL
};

// the next power of two >= e (e >= 1)
static inline int irrl_eval_ensemble_padded(int e) {
  int p = 1;
  while (p < e) p <<= 1;
  return p;
}

// one launch of irrl_eval_ensemble_kernel over (F, C) workgroups on `stream`; the arguments have been checked (F >= 1, C >= 1)
hipError_t irrl_eval_ensemble_launch(const EnsembleArgs &a, hipStream_t stream);
