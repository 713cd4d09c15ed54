"""ctypes binding of libirrl_env.so (include/irrl_env.h).  Fails loudly: there is no fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IRRL_ENV_LIB") or os.path.join(_HERE, "libirrl_env.so")  # override: A/B builds of the same ABI
_lib = None

fp = C.POINTER(C.c_float)
dp = C.POINTER(C.c_double)
u8 = C.POINTER(C.c_uint8)
vp = C.c_void_p

# name -> (restype, argtypes); exactly the symbols declared in include/irrl_env.h
SIGNATURES = {
    "irrl_last_error": (C.c_char_p, []),
    "irrl_version": (C.c_char_p, []),
    "irrl_env_create": (vp, [C.c_char_p, C.c_char_p, C.c_int]),
    "irrl_env_destroy": (None, [vp]),
    "irrl_env_init": (C.c_int, [vp]),
    "irrl_env_set_stream": (C.c_int, [vp, vp]),
    "irrl_env_num_envs": (C.c_int, [vp]),
    "irrl_env_lanes_per_robot": (C.c_int, [vp]),
    "irrl_env_waves_per_simd": (C.c_int, [vp]),
    "irrl_env_ob_dim": (C.c_int, [vp]),
    "irrl_env_action_dim": (C.c_int, [vp]),
    "irrl_env_extra_dim": (C.c_int, [vp]),
    "irrl_env_extra_name": (C.c_char_p, [vp, C.c_int]),
    "irrl_kernel_variant_for": (C.c_char_p, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int]),
    "irrl_env_kernel_variant": (C.c_char_p, [vp]),
    "irrl_env_kernel_name": (C.c_char_p, [vp, C.c_int]),
    "irrl_env_persistent_supported": (C.c_int, [vp]),
    "irrl_env_step": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "irrl_env_step_host": (C.c_int, [vp, fp, fp, fp, u8, fp]),
    "irrl_env_step_rows": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "irrl_env_step_rows_persistent": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "irrl_env_step_rows_out": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "irrl_env_step_rows_persistent_out": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "irrl_env_test_step_host": (C.c_int, [vp, fp, fp, fp, u8, fp]),
    "irrl_env_reset": (C.c_int, [vp, vp]),
    "irrl_env_reset_host": (C.c_int, [vp, fp]),
    "irrl_env_observe": (C.c_int, [vp, vp]),
    "irrl_env_observe_host": (C.c_int, [vp, fp]),
    "irrl_env_is_terminal": (C.c_int, [vp, vp]),
    "irrl_env_is_terminal_host": (C.c_int, [vp, u8]),
    "irrl_env_set_seed": (C.c_int, [vp, C.c_int]),
    "irrl_env_set_simulation_dt": (C.c_int, [vp, C.c_double]),
    "irrl_env_set_control_dt": (C.c_int, [vp, C.c_double]),
    "irrl_env_close": (C.c_int, [vp]),
    "irrl_env_curriculum_update": (C.c_int, [vp]),
    "irrl_env_origin_state_host": (C.c_int, [vp, fp]),
    "irrl_env_reference_state_host": (C.c_int, [vp, fp]),
    "irrl_env_joint_effort_host": (C.c_int, [vp, fp]),
    "irrl_env_generalized_force_host": (C.c_int, [vp, fp]),
    "irrl_env_inverse_mass_matrix_host": (C.c_int, [vp, fp]),
    "irrl_env_nonlinear_host": (C.c_int, [vp, fp]),
    "irrl_env_set_contact_coeff_host": (C.c_int, [vp, fp]),
    "irrl_env_sphere_info_host": (C.c_int, [vp, fp]),
    "irrl_env_get_state_host": (C.c_int, [vp, dp]),
    "irrl_env_set_state_host": (C.c_int, [vp, dp]),
    "irrl_env_heightfield_host": (C.c_int, [vp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "irrl_env_set_ref_host": (C.c_int, [vp, fp, C.c_int, C.c_int]),
    "irrl_env_cfg_value": (C.c_double, [vp, C.c_char_p]),
    "irrl_env_counters_host": (C.c_int, [vp, C.POINTER(C.c_ulonglong)]),
    "irrl_env_counters": (C.c_int, [vp, vp]),
    "irrl_env_snapshot": (C.c_int, [vp]),
    "irrl_env_restore": (C.c_int, [vp]),
    "irrl_bench_actions": (C.c_int, [C.c_uint, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_float, vp, vp]),
    "irrl_gae": (C.c_int, [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp]),
    "irrl_calib_copy_dword": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "irrl_ppo_loss": (C.c_int, [C.c_size_t, C.c_int] + [vp] * 8 + [C.c_float, C.c_float] + [vp] * 3 + [C.c_int, vp]),
    "irrl_ppo_heads_loss": (C.c_int, [C.c_size_t, C.c_int, C.c_int] + [vp] * 12 + [C.c_float, C.c_float] + [vp] * 5 + [C.c_int, vp]),
    "irrl_mlp_ppo_grads": (C.c_int, [C.c_int, C.c_size_t, vp, C.c_int, C.c_int, C.c_int] + [vp] * 13 + [C.c_float, C.c_float, vp, C.c_int, vp]),
    "irrl_mlp_ppo_grads_bf16": (C.c_int, [C.c_int, C.c_size_t, vp, C.c_int, C.c_int, C.c_int] + [vp] * 13 + [C.c_float, C.c_float, vp, C.c_int, vp]),
    "irrl_mlp_ppo_partial_len": (C.c_int, []),
    "irrl_adv_moments": (C.c_int, [C.c_size_t, vp, vp, vp, vp, C.c_int, vp, vp, vp]),
    "irrl_mlp_pack_records": (C.c_int, [C.c_size_t, vp, vp, vp, vp, vp, vp, vp]),
    "irrl_mlp_record_floats": (C.c_int, []),
    "irrl_mlp_ppo_grads_bf16_rec": (C.c_int, [C.c_int, C.c_size_t, vp, vp] + [vp] * 8 + [C.c_float, C.c_float, vp, C.c_int, vp]),
    "irrl_adv_moments_rec": (C.c_int, [C.c_size_t, vp, vp, vp, C.c_int, vp, vp, vp]),
    "irrl_sum_rows": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "irrl_lstm_seq_forward_bf16": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 11),
    "irrl_lstm_seq_backward_bf16": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 15),
    "irrl_clip_adam": (C.c_int, [C.c_int, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_longlong, vp, vp]),
    "irrl_sum_rows_scatter": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "irrl_random_permutation": (C.c_int, [C.c_longlong, C.c_uint, C.c_uint, vp, vp]),
    "irrl_lstm_seq_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "irrl_lstm_seq_forward_x": (C.c_int, [C.c_int] * 4 + [vp] * 11),
    "irrl_lstm_seq_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "irrl_lstm_seq_backward_x": (C.c_int, [C.c_int] * 4 + [vp] * 14),
    "irrl_mlp_policy_step": (C.c_int, [C.c_int] * 4 + [vp] * 9 + [C.c_int, C.c_uint, C.c_longlong, vp, C.c_int] + [vp] * 4 + [C.c_longlong] + [vp] * 8),
    "irrl_lstm_policy_step": (C.c_int, [C.c_int] * 4 + [vp] * 11 + [C.c_int, C.c_uint, C.c_longlong, vp, C.c_int] + [vp] * 4 + [C.c_longlong] + [vp] * 8),
    "irrl_mlp_rollout": (C.c_int, [vp] + [C.c_int] * 4 + [vp] * 9 + [C.c_int, C.c_uint, C.c_longlong, vp, C.c_int] + [vp] * 4 + [C.c_longlong] + [vp] * 8 + [C.c_int, vp]),
    "irrl_lstm_rollout_supports": (C.c_int, [vp, C.c_int, C.c_int]),
    "irrl_mlp_rollout_supports": (C.c_int, [vp, C.c_int, C.c_int]),
    "irrl_lstm_rollout": (C.c_int, [vp] + [C.c_int] * 4 + [vp] * 11 + [C.c_int, C.c_uint, C.c_longlong, vp, C.c_int] + [vp] * 4 + [C.c_longlong] + [vp] * 8 + [C.c_int, vp]),
    # handle, steps, step0, hid, ob, act | weight table + 5 head arrays | depth, 7 state arrays, work | delay, cmd_target | a_cmd, a_vel, a_act,
    # cmd_mean, cmd_std (host), clip | 8 recorders, stats | stream
    "irrl_lstm_eval_rollout": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3 + [fp, fp, C.c_int]
                               + [vp] * 9 + [vp]),
    # the same loop as one persistent launch: the same argument list
    "irrl_lstm_eval_rollout_persistent": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                                          + [fp, fp, C.c_int] + [vp] * 9 + [vp]),
    "irrl_lstm_eval_rollout_supports": (C.c_int, [vp, C.c_int]),
    # both forms with a scenario: the same argument list with `const irrl_eval_scenario *` (EvalScenario below; None = NULL = the old call) in
    # front of the stream
    "irrl_lstm_eval_scenario": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                                + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp]),
    "irrl_lstm_eval_scenario_persistent": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                                           + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp]),
    # both forms with a kick table: the scenario's list with `const irrl_eval_kicks *` (EvalKicks below; None = NULL = the scenario call) behind
    # the scenario
    "irrl_lstm_eval_perturbed": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                                 + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp]),
    "irrl_lstm_eval_perturbed_persistent": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                                            + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp]),
    # both forms with the gait measurements: the kick call's list with `const irrl_eval_gait *` (EvalGait below; None = NULL = the kick call)
    # behind the kicks
    "irrl_lstm_eval_measured": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                                + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp, vp]),
    "irrl_lstm_eval_measured_persistent": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                                           + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp, vp]),
    # the loop with MlpPolicy as the actor, both forms: irrl_lstm_eval_measured's list with the table of 8 where lstm_w is and without lstm_state
    "irrl_mlp_eval_measured": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 7 + [vp] * 2 + [C.c_float] * 3
                               + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp, vp]),
    "irrl_mlp_eval_measured_persistent": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 7 + [vp] * 2 + [C.c_float] * 3
                                          + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp, vp]),
    "irrl_mlp_eval_rollout_supports": (C.c_int, [vp, C.c_int]),
    # one kick row per env on the pool now: device rows [N, 11] / host rows
    "irrl_env_perturb_base": (C.c_int, [vp, vp]),
    "irrl_env_perturb_base_host": (C.c_int, [vp, fp]),
    # the ensemble analysis of a body recorder: rec_body, rows, num_envs, conditions, explorations, frame_first, frame_every, frames | mask |
    # `const irrl_eval_ensemble_spec *` (EvalEnsembleSpec below) | entropy, counts, hist, moments | stream
    "irrl_eval_ensemble": (C.c_int, [vp] + [C.c_int] * 7 + [vp, vp] + [vp] * 4 + [vp]),
    # the recurrence analysis of a body recorder: rec_body, rows, num_envs, frame_first, frame_every, frames |
    # `const irrl_eval_recurrence_spec *` (EvalRecurrenceSpec below) | counts, lag, matrix | stream
    "irrl_eval_recurrence": (C.c_int, [vp] + [C.c_int] * 5 + [vp] + [vp] * 3 + [vp]),
    # the footfall analysis of a gait recorder: rec_gait, rec_done | rows, num_envs, frame_first, frame_every, frames |
    # `const irrl_eval_footfall_spec *` (EvalFootfallSpec below) | counts, support, phase, pattern | stream
    "irrl_eval_footfall": (C.c_int, [vp, vp] + [C.c_int] * 5 + [vp] + [vp] * 4 + [vp]),
    # the motor plane of a gait recorder: rec_gait, rec_done | rows, num_envs, conditions, robots, frame_first, frame_every, frames |
    # `const irrl_eval_motor_spec *` (EvalMotorSpec below) | counts, hist, fold | stream
    "irrl_eval_motor_plane": (C.c_int, [vp, vp] + [C.c_int] * 7 + [vp] + [vp] * 3 + [vp]),
    # the five-launch loop with trace recorders: the measured calls' lists with `const irrl_eval_trace *` (EvalTrace below; None = NULL = the
    # measured call) behind the gait measurements
    "irrl_lstm_eval_traced": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 8 + [vp] * 2 + [C.c_float] * 3
                              + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp, vp, vp]),
    "irrl_mlp_eval_traced": (C.c_int, [vp, C.c_int, C.c_longlong] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] + [vp] * 7 + [vp] * 2 + [C.c_float] * 3
                             + [fp, fp, C.c_int] + [vp] * 9 + [vp, vp, vp, vp, vp]),
    # the correlation moments of two recorder windows: x, y, rec_done | rows, num_envs, conditions, robots, frame_first, frame_every, frames |
    # `const irrl_eval_corr_spec *` (EvalCorrSpec below) | count, sx, sy, sxy, range_x, range_y, work | stream
    "irrl_eval_correlation": (C.c_int, [vp, vp, vp] + [C.c_int] * 7 + [vp] + [vp] * 7 + [vp]),
    "irrl_eval_correlation_work": (C.c_size_t, [C.c_int, vp]),
    # the spectrogram and Welch spectrum of recorder columns: x, rec_done | rows, num_envs, conditions, robots, frame_first, frame_every, frames |
    # `const irrl_eval_spectrum_spec *` (EvalSpectrumSpec below) | window, tw | segments, psd_sum, sxx, work | stream
    "irrl_eval_spectrum": (C.c_int, [vp, vp] + [C.c_int] * 7 + [vp] + [vp] * 2 + [vp] * 4 + [vp]),
    "irrl_eval_spectrum_work": (C.c_size_t, [C.c_int, vp]),
    # HOST tables for it: nperseg, window_kind (0 boxcar, 1 Hann, 2 Tukey), alpha | window [nperseg], tw [nperseg, 2]
    "irrl_eval_spectrum_tables": (C.c_int, [C.c_int, C.c_int, C.c_double, dp, dp]),
}


class EvalScenario(C.Structure):
    """struct irrl_eval_scenario of include/irrl_env.h (a HOST struct of scalars and device pointers); pass C.byref(...) or None"""
    _fields_ = [("t0", C.c_longlong), ("cmd_rows", C.c_int), ("cmd_every", C.c_int), ("cmd_table", vp), ("stat_buckets", C.c_int), ("stat_every", C.c_int),
                ("heading_ref", vp), ("heading_kp", vp), ("heading_ki", vp), ("heading_int", vp), ("heading_windup", C.c_float), ("heading_dt", C.c_float)]


class EvalKicks(C.Structure):
    """struct irrl_eval_kicks of include/irrl_env.h (a HOST struct; kick_table a device pointer to [kick_rows, N, 11] f32); C.byref(...) or None"""
    _fields_ = [("kick_rows", C.c_int), ("kick_first", C.c_longlong), ("kick_every", C.c_int), ("kick_table", vp)]


class EvalGait(C.Structure):
    """struct irrl_eval_gait of include/irrl_env.h (a HOST struct of device pointers: gait f64 [stat_buckets, IRRL_EVAL_GAIT_COUNT, N], prev_contact u8
    [N, 4], rec_gait f32 [steps, N, 32]); C.byref(...) or None"""
    _fields_ = [("gait", vp), ("prev_contact", vp), ("rec_gait", vp)]


class EvalEnsembleSpec(C.Structure):
    """struct irrl_eval_ensemble_spec of include/irrl_env.h (a HOST struct of scalars: the entropy cells lb / ub / prec and the histogram ranges
    per feature, hist_bins = 0 for no histograms); C.byref(...)"""
    _fields_ = [("lb", C.c_double * 6), ("ub", C.c_double * 6), ("prec", C.c_double * 6), ("hist_lo", C.c_double * 6), ("hist_hi", C.c_double * 6),
                ("hist_bins", C.c_int)]


class EvalRecurrenceSpec(C.Structure):
    """struct irrl_eval_recurrence_spec of include/irrl_env.h (a HOST struct of scalars: the box lb / ub, the level width eps, the number of
    levels, the recurrence radius in levels, the Theiler window, the shortest diagonal / vertical line, the number of lag words, the robots whose
    matrices are wanted); C.byref(...)"""
    _fields_ = [("lb", C.c_double * 6), ("ub", C.c_double * 6), ("eps", C.c_double), ("steps", C.c_int), ("radius", C.c_int), ("theiler", C.c_int),
                ("lmin", C.c_int), ("vmin", C.c_int), ("lags", C.c_int), ("matrix_count", C.c_int), ("matrix_env", C.c_int * 8)]


class EvalFootfallSpec(C.Structure):
    """struct irrl_eval_footfall_spec of include/irrl_env.h (a HOST struct: the dilation's reach and the hold in frames, the phase bins)"""
    _fields_ = [("reach", C.c_int), ("hold", C.c_int), ("phase_bins", C.c_int)]


class EvalMotorSpec(C.Structure):
    """struct irrl_eval_motor_spec of include/irrl_env.h (a HOST struct: the motor envelope, the knee's gear ratio, the saturation band, the
    histogram's ranges and bins, the fold's period in frames)"""
    _fields_ = [(k, C.c_double) for k in ("tau_max", "w_crit", "w_max", "knee_ratio", "sat", "t_lo", "t_hi", "w_lo", "w_hi")] + \
               [(k, C.c_int) for k in ("t_bins", "w_bins", "period")]


class EvalTrace(C.Structure):
    """struct irrl_eval_trace of include/irrl_env.h (a HOST struct of device pointers: rec_lstm f32 [steps, N, 4 hid], the actor's half of the
    recurrent state after each policy step; rec_value f32 [steps, N], the critic's value); C.byref(...) or None"""
    _fields_ = [("rec_lstm", vp), ("rec_value", vp)]


class EvalCorrSpec(C.Structure):
    """struct irrl_eval_corr_spec of include/irrl_env.h (a HOST struct: row width, first column and column count of the x and of the y window)"""
    _fields_ = [(k, C.c_int) for k in ("x_dim", "x_first", "x_count", "y_dim", "y_first", "y_count")]


class EvalSpectrumSpec(C.Structure):
    """struct irrl_eval_spectrum_spec of include/irrl_env.h (a HOST struct: row width, first column and column count of the window, the segment
    length and hop in frames, the detrend switch, the robots whose spectrograms are wanted, the sampling rate, the scale per analysed column)"""
    _fields_ = [(k, C.c_int) for k in ("x_dim", "x_first", "x_count", "nperseg", "hop", "detrend", "matrix_count")] + \
               [("matrix_env", C.c_int * 8), ("fs", C.c_double), ("scale", C.c_double * 64)]


def load():
    """Load the HIP library.  Raises if it has not been built -- build it with
    ``python -m high_speed_quadrupedal_locomotion_by_irrl_amd.build`` (or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libirrl_env.so is missing: build the gfx950 extension first "
                           "(python -m high_speed_quadrupedal_locomotion_by_irrl_amd.build). "
                           "There is no CPU or PyTorch fallback for the env kernels.")
    # PyTorch-ROCm is the device-memory / stream plumbing of this engine and ships its own HIP runtime
    # (libamdhip64).  Import it BEFORE dlopen-ing the kernels so that the process holds exactly one HIP runtime
    # (two copies in one process cannot both open the device: the second one sees no GPU).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def version():
    """"gfx950;irrl-env rN;irrl-src-hash:<hex>" of the loaded library (the hash covers every source under csrc/ + the flags)"""
    return load().irrl_version().decode()


def last_error():
    return load().irrl_last_error().decode("utf-8", "replace")


# Two ways an entry point reports a failure (written down here once):
#   * csrc/irrl_env_abi.hip -- every irrl_env_*, irrl_lstm_rollout / irrl_mlp_rollout and their *_supports queries (< 0), irrl_gae, irrl_ppo_loss,
#     irrl_ppo_heads_loss, irrl_mlp_ppo_grads*, irrl_mlp_pack_records, irrl_adv_moments*, irrl_clip_adam, irrl_sum_rows_scatter,
#     irrl_random_permutation, irrl_bench_actions, irrl_calib_copy_dword -- SETS the text of irrl_last_error(): `check(rc)`;
#   * csrc/lstm_kernels.hip -- irrl_lstm_seq_forward[_x|_bf16], irrl_lstm_seq_backward[_x|_bf16], irrl_lstm_policy_step, irrl_mlp_policy_step,
#     irrl_sum_rows -- returns non-zero and nothing else (irrl_last_error() would be some earlier call's text): `check_rc(rc, name, **dims)`.
def check(rc):
    if rc != 0:
        raise RuntimeError("irrl_env: " + last_error())


def check_rc(rc, name, **dims):
    if rc != 0:
        raise RuntimeError("%s failed (rc=%d%s)" % (name, rc, "".join(", %s=%s" % kv for kv in dims.items())))


# argument marshalling: the one place where tensors and streams turn into C pointers
def ptr(t):
    """address of a tensor's first element; None stays None (the C side sees NULL: an optional argument)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device):
    """torch's current stream on `device`: every launch of the library is ordered on it (and recorded by a graph capture)"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def contig(t):
    return t if t.is_contiguous() else t.contiguous()
