// env_kernels_decl.h -- the signatures of the env kernels, included by their definitions (env_kernels.hip) and by the launcher
// (irrl_env_abi.hip).  The kernels are extern "C": a definition that drifts from its declaration here does not compile, where two
// hand-kept copies would link and launch with a wrong kernarg layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "env_params.h"
struct PolicyStepArgs;   // policy_step.hpp
struct EvalArgs;         // eval_elements.hpp

// The env kernels are compiled in two lane layouts from the same source (csrc/env_kernels.hip, see build.py):
//   _l16  16 lanes per robot (lanes_hip16.hpp): 4 robots per wave -- fills all 1024 SIMDs at 4096 robots, shortest step
//   _l4    4 lanes per robot (lanes_hip.hpp):  16 robots per wave -- 2.3x fewer instructions per robot, the better
//          throughput once the pool is large enough to occupy the chip on its own
//   _l4w2  the same, compiled for two waves per SIMD (256 registers each): pools with more 4-lane waves than SIMDs (> 16 384 robots)
#define IRRL_STEP_KERNEL_ARGS EnvParams, EnvState, const float *, float *, float *, uint8_t *, float *
#define IRRL_STEPS_KERNEL_ARGS EnvParams, EnvState, const float *, int, int, int, float *, float *, uint8_t *, float *, int
#define IRRL_ROLLOUT_KERNEL_ARGS EnvParams, EnvState, float *, float *, uint8_t *, float *, PolicyStepArgs, int
#define IRRL_DECLARE_KERNELS(sfx)                                                          \
  extern "C" __global__ void irrl_step_kernel##sfx(IRRL_STEP_KERNEL_ARGS);                 \
  extern "C" __global__ void irrl_step_kernel_dir##sfx(IRRL_STEP_KERNEL_ARGS);             \
  extern "C" __global__ void irrl_step_kernel_md##sfx(IRRL_STEP_KERNEL_ARGS);              \
  extern "C" __global__ void irrl_step_kernel_crutial##sfx(IRRL_STEP_KERNEL_ARGS);         \
  extern "C" __global__ void irrl_step_kernel_crutial_md##sfx(IRRL_STEP_KERNEL_ARGS);      \
  extern "C" __global__ void irrl_step_kernel_flat##sfx(IRRL_STEP_KERNEL_ARGS);            \
  extern "C" __global__ void irrl_steps_persistent_kernel##sfx(IRRL_STEPS_KERNEL_ARGS);    \
  extern "C" __global__ void irrl_steps_persistent_kernel_flat##sfx(IRRL_STEPS_KERNEL_ARGS); \
  extern "C" __global__ void irrl_steps_persistent_kernel_rt##sfx(IRRL_STEPS_KERNEL_ARGS); \
  extern "C" __global__ void irrl_steps_persistent_kernel_dir##sfx(IRRL_STEPS_KERNEL_ARGS); \
  extern "C" __global__ void irrl_init_kernel##sfx(EnvParams, EnvState);                   \
  extern "C" __global__ void irrl_reset_kernel##sfx(EnvParams, EnvState, float *);         \
  extern "C" __global__ void irrl_observe_kernel##sfx(EnvParams, EnvState, float *);       \
  extern "C" __global__ void irrl_probe_kernel##sfx(EnvParams, EnvState, float *, float *);
IRRL_DECLARE_KERNELS(_l16)
IRRL_DECLARE_KERNELS(_l4)
IRRL_DECLARE_KERNELS(_l4w2)
#undef IRRL_DECLARE_KERNELS
extern "C" __global__ void irrl_terminal_kernel(EnvParams, EnvState, uint8_t *);
// the kernels with the policy in the same launch (16-lane layout; csrc/env_rollout_kernels.hpp): sfx _l16 = the shipped solver settings compiled in,
// _rt_l16 = read from EnvParams
#define IRRL_DECLARE_ROLLOUT_KERNELS(sfx)                                                                      \
  extern "C" __global__ void irrl_step_policy_kernel##sfx(IRRL_STEP_KERNEL_ARGS, PolicyStepArgs);              \
  extern "C" __global__ void irrl_rollout_persistent_kernel##sfx(IRRL_ROLLOUT_KERNEL_ARGS);                    \
  extern "C" __global__ void irrl_rollout_persistent_actor_kernel##sfx(IRRL_ROLLOUT_KERNEL_ARGS);              \
  extern "C" __global__ void irrl_rollout_persistent_actor_wave_kernel##sfx(IRRL_ROLLOUT_KERNEL_ARGS);         \
  extern "C" __global__ void irrl_rollout_persistent_mlp_kernel##sfx(IRRL_ROLLOUT_KERNEL_ARGS);
IRRL_DECLARE_ROLLOUT_KERNELS(_l16)
IRRL_DECLARE_ROLLOUT_KERNELS(_rt_l16)
#undef IRRL_DECLARE_ROLLOUT_KERNELS
// the whole policy evaluation in one launch (16-lane layout; csrc/env_eval_kernels.hpp, a translation unit of its own): same suffixes
#define IRRL_EVAL_KERNEL_ARGS EnvParams, EnvState, float *, float *, uint8_t *, float *, PolicyStepArgs, EvalArgs
extern "C" __global__ void irrl_eval_persistent_kernel_l16(IRRL_EVAL_KERNEL_ARGS);
extern "C" __global__ void irrl_eval_persistent_kernel_rt_l16(IRRL_EVAL_KERNEL_ARGS);
// the same with MlpPolicy as the actor (csrc/env_eval_mlp_kernels.hpp, a translation unit of its own)
extern "C" __global__ void irrl_eval_mlp_persistent_kernel_l16(IRRL_EVAL_KERNEL_ARGS);
extern "C" __global__ void irrl_eval_mlp_persistent_kernel_rt_l16(IRRL_EVAL_KERNEL_ARGS);
