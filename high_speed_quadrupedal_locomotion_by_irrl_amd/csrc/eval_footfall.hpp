// eval_footfall.hpp -- what the C-ABI (irrl_env_abi.hip: irrl_eval_footfall and irrl_eval_motor_plane, which check the arguments) and the
// kernels' translation unit (eval_footfall.hip) share: the kernels' argument blocks and their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include "eval_elements.hpp"

struct FootfallArgs {
  const float *rec_gait;       // [rows, N, 32]
  const uint8_t *rec_done;     // [rows, N] or NULL
  int N, T;                    // pool size = the grid; analysed frames per robot (1 .. IRRL_EVAL_FOOTFALL_MAX_FRAMES)
  int frame_first, frame_every;
  irrl_eval_footfall_spec spec;
  uint32_t *counts;            // [N, 4, 14]
  uint32_t *support;           // [N, 16] or NULL
  uint32_t *phase;             // [N, 3, spec.phase_bins] or NULL
  uint8_t *pattern;            // [T, N] or NULL
};

struct MotorPlaneArgs {
  const float *rec_gait;       // [rows, N, 32]
  const uint8_t *rec_done;     // [rows, N] or NULL
  int N, C, R, T;              // pool size, conditions, robots per condition (N = C R), analysed frames
  int frame_first, frame_every;
  irrl_eval_motor_spec spec;
  uint32_t *counts;            // [C, 12, 6]
  uint32_t *hist;              // [C, 12, t_bins, w_bins] or NULL
  double *fold;                // [C, 12, period, 3] or NULL
};

// the 64-frame words of a leg's flags
static inline IRRL_EVAL_FN int irrl_eval_footfall_words(int T) { return (T + 63) / 64; }

// one launch each over N workgroups / C * 12 workgroups on `stream`; the arguments have been checked (T >= 1)
hipError_t irrl_eval_footfall_launch(const FootfallArgs &a, hipStream_t stream);
hipError_t irrl_eval_motor_plane_launch(const MotorPlaneArgs &a, hipStream_t stream);
