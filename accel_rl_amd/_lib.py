"""ctypes binding of libaccel_rl_hip.so (include/accel_rl_hip.h).

There is NO fallback: if the shared library is missing or a call fails, the
product raises.  PyTorch is used only as the owner of device memory and
streams; the ABI itself sees raw pointers and sizes.
"""
import collections
import ctypes as C
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libaccel_rl_hip.so")

ARL_ABI_VERSION = 5
PROMO_NEP50, PROMO_LEGACY, PROMO_ASSOC = 0, 1, 2
PPO_TIE_THEANO, PPO_TIE_MATH, PPO_TIE_BOTH = 0, 1, 2      # ARL_PPO_TIE_*: whose gradient min() / clip() hand on (accel_rl_hip.h)
PPG_POLICY, PPG_AUX = 0, 1                                # ARL_PPG_*: arl_ppg_head_loss_parts' phase
OPT_ADAM, OPT_RMSPROP = 0, 1
VMPO_MAX_ROWS = 65536                                     # ARL_VMPO_MAX_ROWS: rows of one arl_vmpo_weights launch
RND_MAX_ROWS, RND_MIX_MAX_ENVS, RND_MIX_MAX_ROWS = 1 << 24, 1 << 20, 1 << 22   # ARL_RND_MAX_ROWS, ARL_RND_MIX_MAX_*
POPART_MAX_ROWS, POPART_MAX_HID = 1 << 22, 1 << 16        # ARL_POPART_MAX_ROWS, ARL_POPART_MAX_HID
MAX_ACTIONS = 18
REPLAY_MAX_HORIZON = 16
RAW_H, RAW_W, OBS_H, OBS_W = 210, 160, 104, 80
OPT_PARTIALS = 1024

_vp, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double


class ArlGame(C.Structure):
    _fields_ = [("bank", _vp), ("n_frames", _i32), ("n_actions", _i32),
                ("action_set", _i32 * MAX_ACTIONS), ("start_lives", _i32),
                ("life_period", _i32), ("frame_skip", _i32), ("n_stack", _i32),
                ("clip_reward", _i32), ("episodic_lives", _i32), ("resample_mode", _i32)]


RESAMPLE_BOX2X, RESAMPLE_NEAREST = 0, 1       # ARL_RESAMPLE_* (atari_env.py:155; box2x = what the reference computes)
RESAMPLE_MODES = dict(box2x=RESAMPLE_BOX2X, nearest=RESAMPLE_NEAREST)


EPOCH_WORDS = 32 * 17         # ARL_EPOCH_WORDS: launch epoch + arl_env_step's arrival tickets


class ArlEnvState(C.Structure):
    _fields_ = [("n_env", _i64), ("tick", _vp), ("emu_lives", _vp), ("env_lives", _vp),
                ("phase", _vp), ("over", _vp), ("frozen", _vp),
                ("traj_len", _vp), ("traj_nonzero", _vp), ("traj_ret", _vp),
                ("traj_raw", _vp), ("traj_disc", _vp), ("traj_curdisc", _vp),
                ("frame_a", _vp), ("frame_b", _vp), ("frame_mode", _vp), ("reset_flag", _vp),
                ("noop_ring", _vp), ("noop_cursor", _vp), ("epoch", _vp),
                ("noop_ring_len", _i32), ("envs_per_stream", _i32),
                ("done_count", _vp), ("done_int", _vp), ("done_flt", _vp),
                ("done_capacity", _i32), ("next_reset", _vp), ("launch_count", _vp)]


class ArlRollout(C.Structure):
    _fields_ = [("horizon", _i32), ("observations", _vp), ("rewards", _vp), ("dones", _vp),
                ("raw_reward", _vp), ("need_reset", _vp), ("actions", _vp), ("prob", _vp),
                ("value", _vp), ("step_obs", _vp)]


class ArlConvGeom(C.Structure):
    _fields_ = [("batch", _i64), ("in_h", _i32), ("in_w", _i32), ("in_c", _i32), ("out_c", _i32),
                ("kh", _i32), ("kw", _i32), ("stride", _i32), ("pad_h", _i32), ("pad_w", _i32), ("route", _i32)]


class ArlCorunJob(C.Structure):
    _fields_ = [("opaque", _i64 * 40)]


class ArlFoldItem(C.Structure):
    _fields_ = [("part", _vp), ("out", _vp), ("total", _i64), ("splits", _i32), ("valid", _i32)]


FOLD_MAX_ITEMS = 24


class ArlWgradPlan(C.Structure):
    _fields_ = [("opaque", _i64 * 32)]


WGRAD_GROUP_MAX = 4


class ArlLogitSrc(C.Structure):
    _fields_ = [("part", _vp), ("bias_or_null", _vp), ("split_stride", _i64), ("splits", _i32), ("reserved", _i32)]


class ArlDgradWt(C.Structure):
    _fields_ = [("w", _vp), ("wt", _vp), ("geom", C.POINTER(ArlConvGeom))]


DGRAD_WT_MAX = 4


class ArlServeHead(C.Structure):
    _fields_ = [("hidden", ArlFoldItem), ("hidden_bias", _vp), ("hidden_relu", _i32), ("hid", _i32),
                ("w_head", _vp), ("b_head", _vp), ("hidden_out", _vp)]


class ArlServeConv1(C.Structure):
    _fields_ = [("geom", C.POINTER(ArlConvGeom)), ("w", _vp), ("bias", _vp), ("y", _vp), ("scale", _f32),
                ("relu", _i32)]


class ArlGatherItem(C.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("row_bytes", _i64), ("src_rows", _i64)]


GATHER_MAX_ITEMS = 8
ROW_MAP_IDENTITY, ROW_MAP_STEP_MAJOR = 0, 1       # ARL_ROW_MAP_*


class ArlRowMap(C.Structure):
    _fields_ = [("kind", _i32), ("horizon", _i32), ("n_env", _i32), ("reserved", _i32)]


class ArlNoisyLayer(C.Structure):
    _fields_ = [("fein", _vp), ("feout", _vp), ("x", _vp), ("xs", _vp), ("fan_in", _i32), ("units", _i32),
                ("out_stride", _i32), ("layer", _i32)]


NOISY_MAX_LAYERS = 8


class ArlNoisyDraw(C.Structure):
    _fields_ = [("f", _vp), ("x", _vp), ("xs", _vp), ("width", _i32), ("pitch", _i32), ("layer", _i32),
                ("which", _i32)]


NOISY_MAX_DRAWS = 16


class ArlNoisyLogitSrc(C.Structure):
    _fields_ = [("w_part", _vp), ("bias_or_null", _vp), ("s_part", _vp), ("b_sigma_or_null", _vp), ("feout", _vp),
                ("w_split_stride", _i64), ("s_split_stride", _i64), ("w_splits", _i32), ("s_splits", _i32)]


class ArlReplay(C.Structure):
    _fields_ = [("n_env", _i64), ("size", _i32), ("n_stack", _i32), ("frame_bytes", _i32),
                ("reward_horizon", _i32), ("frames", _vp), ("n_blanks", _vp), ("acts", _vp),
                ("terminals", _vp), ("rewards", _vp), ("returns", _vp)]


class ArlOptState(C.Structure):
    _fields_ = [("n_params", _i64), ("params", _vp), ("grads", _vp), ("slot0", _vp),
                ("slot1", _vp), ("step_count", _vp), ("lr_mult", _vp), ("partials", _vp),
                ("grad_norm_log", _vp), ("norm_log_len", _i32)]


_SIGNATURES = {
    "arl_abi_version": (_i32, []),
    "arl_last_error": (C.c_char_p, []),
    "arl_gae_scan": (_i32, [_vp, _vp, _vp, _vp, _f64, _f64, _i64, _i32, _i32, _vp, _vp, _vp]),
    "arl_nstep_return": (_i32, [_vp, _vp, _vp, _vp, _f64, _i64, _i32, _i32, _vp, _vp, _vp]),
    "arl_valids_mask": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "arl_standardize_workspace_bytes": (_i64, []),
    "arl_standardize": (_i32, [_vp, _vp, _i64, _f64, _vp, _vp]),
    "arl_sample_categorical": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "arl_env_act_step": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlEnvState), C.POINTER(ArlRollout),
                                _vp, _vp, _vp, _vp, _i32, _i32, _f64, _f64, _vp]),
    "arl_env_frame_step": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlEnvState), C.POINTER(ArlRollout),
                                  _i32, _i32, _vp]),
    "arl_env_step": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlEnvState), C.POINTER(ArlRollout),
                            _vp, _vp, _vp, _vp, _i32, _i32, _f64, _f64, _i32, _i32, _vp]),
    "arl_rollout_begin": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlEnvState), C.POINTER(ArlRollout), _vp]),
    "arl_env_reset": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlEnvState), C.POINTER(ArlRollout),
                             _vp, _i32, _vp]),
    "arl_preprocess_frames": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "arl_copy_bytes": (_i32, [_vp, _vp, _i64, _vp]),
    "arl_ring_append": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp]),
    "arl_gather_rows_many": (_i32, [C.POINTER(ArlGatherItem), _i32, _vp, _i64, C.POINTER(ArlRowMap), _vp]),
    "arl_gather_scale_obs": (_i32, [_vp, _vp, _i64, _i64, _f32, _vp, _vp]),
    "arl_gather_scale_obs_nhwc": (_i32, [_vp, _vp, _i64, _i32, _i32, _f32, _vp, _vp]),
    "arl_traj_minibatch": (_i32, [_vp, _i32, _i32, _i64, C.POINTER(_vp), _i32, _i32, _vp, _vp, C.POINTER(_vp), _vp, _vp]),
    "arl_bias_relu": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "arl_relu_bwd_workspace_bytes": (_i64, []),
    "arl_relu_bwd_bias_grad": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "arl_pg_head_workspace_bytes": (_i64, []),
    "arl_pg_head_infer": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "arl_pg_head_loss": (_i32, [_vp] * 11 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _i32] + [_vp] * 7),
    "arl_pg_head_loss_parts": (_i32, [_vp] * 11 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _i32] + [_vp] * 7 +
                               [_vp, _i32, _vp]),
    "arl_conv_workspace_bytes": (_i64, []),
    "arl_conv2d_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ArlConvGeom), _i32, _vp, C.POINTER(ArlFoldItem), _vp]),
    "arl_conv2d_bwd_data": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ArlConvGeom), C.POINTER(ArlCorunJob),
                                   C.POINTER(_i32), _vp]),
    "arl_conv2d_dgrad_weights": (_i32, [C.POINTER(ArlDgradWt), _i32, _vp]),
    "arl_conv2d_bwd_weight": (_i32, [_vp, _vp, _vp, C.POINTER(ArlConvGeom), _vp, _vp]),
    "arl_conv2d_bwd_weight_parts": (_i32, [_vp, _vp, _vp, C.POINTER(ArlConvGeom), _vp, _i64, C.POINTER(ArlFoldItem),
                                           _vp, C.POINTER(ArlFoldItem), C.POINTER(ArlWgradPlan), _vp]),
    "arl_fold_many": (_i32, [C.POINTER(ArlFoldItem), _i32, _vp]),
    "arl_conv2d_fwd_plan": (_i32, [C.POINTER(ArlConvGeom), C.POINTER(_i32), C.POINTER(_i32)]),
    "arl_serve_conv1_supported": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlConvGeom)]),
    "arl_rollout_begin_conv1": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlEnvState), C.POINTER(ArlRollout),
                                       C.POINTER(ArlServeConv1), _vp]),
    "arl_env_step_served": (_i32, [C.POINTER(ArlGame), C.POINTER(ArlEnvState), C.POINTER(ArlRollout),
                                   C.POINTER(ArlServeHead), C.POINTER(ArlServeConv1), _vp, _i32, _f64, _f64, _i32, _vp]),
    "arl_conv2d_u8_fwd": (_i32, [_vp, _i64, _vp, _f32, _vp, _vp, _vp, _vp, C.POINTER(ArlConvGeom), _i32, _vp]),
    "arl_conv2d_u8_bwd_weight_parts": (_i32, [_vp, _vp, _i64, _vp, _f32, _vp, C.POINTER(ArlConvGeom), _vp, _i64,
                                              C.POINTER(ArlFoldItem), _vp, C.POINTER(ArlFoldItem),
                                              C.POINTER(ArlWgradPlan), _vp]),
    "arl_conv2d_bwd_pair": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ArlConvGeom), _vp, _i64,
                                   C.POINTER(ArlFoldItem), _vp, C.POINTER(ArlFoldItem), C.POINTER(ArlCorunJob),
                                   C.POINTER(_i32), C.POINTER(ArlWgradPlan), _vp]),
    "arl_conv2d_bwd_weight_group": (_i32, [C.POINTER(ArlWgradPlan), _i32, _vp]),
    "arl_relu_bwd_bias_parts": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, C.POINTER(ArlFoldItem), _vp]),
    "arl_replay_append": (_i32, [C.POINTER(ArlReplay), _vp, _vp, _vp, _vp, _i32, _i32, _f64, _i32, _vp]),
    "arl_replay_extract": (_i32, [C.POINTER(ArlReplay), _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arl_replay_extract_shift": (_i32, [C.POINTER(ArlReplay), _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i64, _i64,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
    "arl_sumtree_find": (_i32, [_vp, _i32, _vp, _i64, _vp, _vp]),
    "arl_sumtree_add": (_i32, [_vp, _i32, _vp, _vp, _i64, _vp]),
    "arl_sumtree_gather": (_i32, [_vp, _vp, _i64, _f64, _vp, _vp]),
    "arl_sumtree_sample": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arl_sumtree_sample_batch": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f64, _vp, _vp, _i32, _vp]),
    "arl_sumtree_update_pow": (_i32, [_vp, _i32, _vp, _vp, _vp, _f64, _i64, _vp]),
    "arl_is_weights": (_i32, [_vp, _i64, _f64, _vp, _vp]),
    "arl_priority_diffs": (_i32, [_vp, _vp, _i64, _f64, _vp, _vp]),
    "arl_catdqn_act": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "arl_catdqn_loss": (_i32, [_vp] * 8 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "arl_catdqn_loss_parts": (_i32, [_vp] * 8 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _i32,
                               _vp]),
    "arl_qrdqn_act": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "arl_qrdqn_loss": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "arl_iqn_embed": (_i32, [_vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "arl_iqn_merge_fwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "arl_iqn_merge_bwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "arl_iqn_act": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "arl_iqn_loss": (_i32, [_vp] * 8 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "arl_miqn_loss": (_i32, [_vp] * 8 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp,
                             _i64, _vp]),
    "arl_fqf_fractions": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arl_fqf_act": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "arl_fqf_loss": (_i32, [_vp] * 13 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arl_dqn_act": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "arl_dqn_loss": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "arl_drq_loss": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "arl_q_regress_loss": (_i32, [_vp] * 4 + [_i64, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "arl_qlambda_scan": (_i32, [_vp] * 4 + [_f64, _f64, _i64, _i32, _i32, _i32, _vp, _vp]),
    "arl_ppg_head_loss_parts": (_i32, [_vp] * 10 + [_i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _i32] +
                                [_vp] * 8),
    "arl_vmpo_weights": (_i32, [_vp, _vp, _i64, _vp, _f64, _vp, _vp, _vp]),
    "arl_vmpo_head_loss_parts": (_i32, [_vp] * 10 + [_i64, _i32, _i32, _f32, _i32] + [_vp] * 8),
    "arl_vmpo_dual_step": (_i32, [_vp] * 7 + [_f32, _i32, _f32, _f32, _f32, _f32, _vp]),
    "arl_vtrace_scan": (_i32, [_vp] * 7 + [_f64] * 5 + [_i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "arl_seq_store": (_i32, [C.POINTER(_vp), _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_vp), _vp, _vp]),
    "arl_seq_prepare": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp, C.POINTER(_vp),
                               _vp, _vp]),
    "arl_r2d2_loss": (_i32, [_vp] * 6 + [_i32] * 7 + [_f64] * 3 + [_vp] * 5),
    "arl_ln_bwd_workspace_bytes": (_i64, []),
    "arl_ln_relu_fwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp]),
    "arl_ln_relu_bwd": (_i32, [_vp] * 5 + [_i64, _i32, _i32, _vp, _vp, _vp, _vp, C.POINTER(ArlFoldItem), _vp]),
    "arl_maxpool3s2_fwd": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "arl_maxpool3s2_bwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "arl_add_relu": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "arl_gather_scale_obs_nhwc_any": (_i32, [_vp, _vp, _i64, _i32, _i32, _f32, _vp, _vp]),
    "arl_mdqn_loss": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "arl_sacd_act": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "arl_sacd_loss": (_i32, [_vp] * 11 + [_i64, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "arl_sacd_alpha_grad": (_i32, [_vp, _i64, _vp, _f32, _vp, _vp]),
    "arl_lstm_cell_fwd": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "arl_lstm_cell_bwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp]),
    "arl_gru_cell_fwd": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp]),
    "arl_gru_cell_bwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp]),
    "arl_rnn_cell_fwd": (_i32, [_vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp]),
    "arl_rnn_cell_bwd": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp]),
    "arl_seq_handover": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp]),
    "arl_lstm_cell_bwd_reset": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp,
                                       _vp, _vp, _i64, _i64, _vp]),
    "arl_gru_cell_bwd_reset": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp,
                                      _vp, _vp, _i64, _i64, _vp]),
    "arl_rnn_cell_bwd_reset": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _vp]),
    "arl_rnd_obs_stats_workspace_bytes": (_i64, [_i32, _i32]),
    "arl_rnd_obs_stats": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "arl_rnd_obs_prepare": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "arl_rnd_error": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "arl_rnd_reward_mix": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _f64, _f64, _f64, _vp, _vp, _vp, _vp]),
    "arl_popart_denorm": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "arl_popart_step": (_i32, [_vp, _vp, _vp, _i64, _f64, _f64, _f64, _vp, _vp, _vp, _i32, _vp, _vp]),
    "arl_acer_retrace_scan": (_i32, [_vp] * 4 + [_i32, _vp, _vp, _vp, _vp, _f64, _f64, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "arl_acer_loss": (_i32, [_vp] * 6 + [_i64, _i32, _i32, _f64, _f64, _f64, _f64, _vp, _vp, _vp]),
    "arl_acer_avg_step": (_i32, [_vp, _vp, _i64, _f32, _vp]),
    "arl_gather_segments": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "arl_opt_step": (_i32, [C.POINTER(ArlOptState), _i32, _f32, _f32, _f32, _f32, _f32, _f32, _vp]),
    "arl_opt_step_noclip": (_i32, [C.POINTER(ArlOptState), _i32, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _vp, _vp]),
    "arl_opt_finish": (_i32, [C.POINTER(ArlOptState), _i32, _f32, _vp, _vp, _vp]),
    "arl_opt_step_noclip_split": (_i32, [C.POINTER(ArlOptState), _i32, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _vp,
                                         _i64, _i64, _i32, _vp]),
    "arl_opt_finish_split": (_i32, [C.POINTER(ArlOptState), _i32, _f32, _vp, _vp, _i64, _vp]),
    "arl_corun_job_init": (_i32, [C.POINTER(ArlCorunJob), C.POINTER(ArlOptState), _i32, _f32, _f32, _f32, _f32, _f32,
                                  _i32, _vp, _vp, _i64, _i64]),
    "arl_corun_job_run": (_i32, [C.POINTER(ArlCorunJob), _vp]),
    "arl_noisy_normals": (_i32, [_i64, _i64, _i32, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "arl_noisy_noise": (_i32, [_vp, C.POINTER(ArlNoisyLayer), _i32, _i64, _i32, _vp]),
    "arl_noisy_dense_combine": (_i32, [C.POINTER(ArlFoldItem), _vp, C.POINTER(ArlFoldItem), _vp, _vp, _i64, _i32, _i32,
                                       _vp, _vp, _vp, _vp, _vp]),
    "arl_noisy_dense_bwd_prep": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "arl_noisy_dense_bwd_dx": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "arl_noisy_draws": (_i32, [_vp, C.POINTER(ArlNoisyDraw), _i32, _i64, _i32, _vp]),
    "arl_noisy_duel_combine": (_i32, [C.POINTER(ArlFoldItem), _vp, C.POINTER(ArlFoldItem), C.POINTER(ArlFoldItem), _vp,
                                      _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "arl_noisy_duel_bwd_prep": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "arl_noisy_duel_bwd_dx": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "arl_noisy_catdqn_loss_limits": (_i32, [C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "arl_noisy_catdqn_loss_parts": (_i32, [C.POINTER(ArlNoisyLogitSrc), C.POINTER(ArlNoisyLogitSrc),
                                           C.POINTER(ArlNoisyLogitSrc), _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32,
                                           _i32, _f32, _f32, _f32, _vp, _vp, _vp, C.POINTER(ArlDgradWt), _i32, _vp]),
}

class ArlDevLaunch(C.Structure):
    _fields_ = [(n, _i32) for n in ("family", "wgm", "wgn", "tm", "tn", "bk", "minw", "flags", "split_mode", "splits")] + \
               [(n, C.c_uint32) for n in ("grid_x", "grid_y", "grid_z", "lds_bytes")]


# include/accel_rl_hip_dev.h: development hooks (tests / tools), not part of the drop-in boundary
_DEV_SIGNATURES = {
    "arl_dev_conv_trace_buffer": (None, [_vp]),
    "arl_dev_conv_force_generic": (None, [_i32]),
    "arl_dev_conv_variant": (None, [_i32]),
    "arl_dev_fwd_tile": (None, [_i32]),
    "arl_dev_dgrad_wt": (None, [_i32]),
    "arl_dev_conv_launch_log": (_i32, [C.POINTER(ArlDevLaunch), _i32]),
    "arl_dev_fold_wide_from": (None, [_i32]),
    "arl_dev_scan_force_wave": (None, [_i32]),
    "arl_dev_scan_wave_groups": (None, [_i32]),
    "arl_dev_env_variant": (None, [_i32]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)
DEV_SYMBOLS = tuple(_DEV_SIGNATURES)

# arl_conv_geom.route (ARL_CONV_ROUTE_*): how the fp32 contractions are computed.  The library keeps no mode; this
# module's default is what conv_geom() / dense_geom() stamp into the geometries they build (host-side policy).
ROUTE_SPLIT9, ROUTE_FP32, ROUTE_SPLIT6, ROUTE_BF16 = 0, 1, 6, 2
_PRECISION_TO_ROUTE = {9: ROUTE_SPLIT9, 0: ROUTE_FP32, 6: ROUTE_SPLIT6, 1: ROUTE_BF16}
default_route = _PRECISION_TO_ROUTE[int(os.environ.get("ARL_CONV_PRECISION", "9"))]    # measurement switch (tools/, bench A/B)


def set_conv_precision(mode):
    """Route of the geometries built from now on: 9 = nine exact bf16-split products (the default), 6 = six,
    0 = the fp32 MFMA chain, 1 = plain bf16 operands (ARL_CONV_ROUTE_BF16: the labelled reduced-precision option, not an
    fp32 contraction).  Geometries already built keep theirs (ArlConvGeom.route)."""
    global default_route
    if mode not in _PRECISION_TO_ROUTE:
        raise ValueError("conv precision: 0 (fp32 MFMA), 6 or 9 (bf16-split products) or 1 (bf16 operands)")
    default_route = _PRECISION_TO_ROUTE[mode]


def conv_precision():
    return {v: k for k, v in _PRECISION_TO_ROUTE.items()}[default_route]

_lib = None


def load():
    """Load (once) and type the shared library.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libaccel_rl_hip.so is not built (%s).  Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `python accel_rl_amd/_build.py`.  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(_SIGNATURES.items()) + list(_DEV_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.arl_abi_version() != ARL_ABI_VERSION:
        raise RuntimeError("libaccel_rl_hip.so ABI %d != binding %d" % (lib.arl_abi_version(), ARL_ABI_VERSION))
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        msg = load().arl_last_error().decode(errors="replace")
        raise RuntimeError("%s failed (code %d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("accel_rl_amd kernels need device (HIP) tensors; got a %s tensor -- "
                           "there is no CPU path" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")
    return t.data_ptr()


def staged_ptr(t):
    """Pointer of a device tensor OR of a pinned host tensor (the device addresses pinned memory directly)."""
    if not (t.is_cuda or t.is_pinned()):
        raise RuntimeError("staging copies take device tensors or PINNED host tensors; got pageable host memory")
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")
    return t.data_ptr()


STAGE_WITH_KERNELS = os.environ.get("ARL_STAGE_KERNELS", "1") != "0"      # (A/B switch: 0 = framework copies = memcpy nodes)


def copy_bytes(dst, src, stream=None):
    """dst <- src as a kernel (a kernel node when captured); either side may be a pinned host tensor."""
    if not STAGE_WITH_KERNELS:
        dst.view(-1).copy_(src.view(-1), non_blocking=True)
        return
    n = src.numel() * src.element_size()
    assert n == dst.numel() * dst.element_size(), "size mismatch"
    _check(load().arl_copy_bytes(staged_ptr(dst), staged_ptr(src), n, stream_ptr(stream)), "arl_copy_bytes")


def ring_append(src, ring, counter, stream=None):
    """ring[counter % len(ring)] = src; counter += 1 (device-side; see arl_ring_append)."""
    _want(src, torch.float32, "src")
    _want(ring, torch.float32, "ring")
    _want(counter, torch.int32, "counter")
    if not (ring.is_contiguous() and src.is_contiguous() and ring.shape[0] > 0 and ring[0].numel() == src.numel()):
        raise ValueError("ring_append: a ring slot must hold exactly the %d floats of src (ring %s)" %
                         (src.numel(), tuple(ring.shape)))
    _check(load().arl_ring_append(ptr(src), src.numel(), ptr(ring), ring.shape[0], ptr(counter), stream_ptr(stream)),
           "arl_ring_append")


def gather_rows_many(pairs, idx, step_major=None, stream=None):
    """dst[j] = src[map(idx[j])] for every (src, dst) of `pairs` (at most GATHER_MAX_ITEMS) in one launch: rows of
    contiguous tensors -- src [src_rows, ...], dst [n_rows, ...] of the same row size and dtype -- picked by one int32
    index vector (None: rows 0 .. n_rows - 1).  step_major = (horizon, n_env): the sources are laid out [horizon][n_env]
    and the indices name rows env-major (env * horizon + t); None: the indices are source rows."""
    if idx is not None:
        _want(idx, torch.int32, "idx")
    n_rows = pairs[0][1].shape[0] if idx is None else idx.numel()
    items = (ArlGatherItem * max(len(pairs), 1))()
    for it, (src, dst) in zip(items, pairs):
        if src.dtype != dst.dtype or dst.shape[0] != n_rows or src[0].numel() != dst[0].numel():
            raise ValueError("gather_rows_many: src %s %s and dst %s %s do not describe the same rows (%d wanted)" %
                             (tuple(src.shape), src.dtype, tuple(dst.shape), dst.dtype, n_rows))
        it.src, it.dst = ptr(src), ptr(dst)
        it.row_bytes, it.src_rows = src[0].numel() * src.element_size(), src.shape[0]
    row_map = None
    if step_major is not None:
        row_map = ArlRowMap(ROW_MAP_STEP_MAJOR, int(step_major[0]), int(step_major[1]), 0)
    _check(load().arl_gather_rows_many(items, len(pairs), ptr(idx), n_rows, None if row_map is None else C.byref(row_map),
                                       stream_ptr(stream)), "arl_gather_rows_many")


def stream_ptr(stream=None):
    s = torch.cuda.current_stream() if stream is None else stream
    return s.cuda_stream


def _want(t, dtype, name):
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))


def _want_flags(t, name):
    if t.dtype not in (torch.uint8, torch.bool):
        raise TypeError("%s must be uint8/bool" % name)


# ---------------------------------------------------------------------------
# thin typed wrappers (device tensors in, device tensors out)
# ---------------------------------------------------------------------------

def gae_scan(rewards, values, dones, last_values, discount, gae_lambda, n_env, horizon,
             advantages, returns, promo=PROMO_NEP50, stream=None):
    for t, n in ((rewards, "rewards"), (values, "values"), (last_values, "last_values"),
                 (advantages, "advantages"), (returns, "returns")):
        _want(t, torch.float32, n)
    _want_flags(dones, "dones")
    assert rewards.numel() == values.numel() == dones.numel() == n_env * horizon
    assert last_values.numel() == n_env and advantages.numel() == returns.numel() == n_env * horizon
    _check(load().arl_gae_scan(ptr(rewards), ptr(values), ptr(dones), ptr(last_values),
                               float(discount), float(gae_lambda), n_env, horizon, promo,
                               ptr(advantages), ptr(returns), stream_ptr(stream)), "arl_gae_scan")


def nstep_return(rewards, dones, values, last_values, discount, n_env, horizon,
                 returns, advantages, promo=PROMO_NEP50, stream=None):
    for t, n in ((rewards, "rewards"), (values, "values"), (last_values, "last_values"),
                 (advantages, "advantages"), (returns, "returns")):
        _want(t, torch.float32, n)
    assert rewards.numel() == values.numel() == dones.numel() == n_env * horizon
    assert last_values.numel() == n_env and advantages.numel() == returns.numel() == n_env * horizon
    _check(load().arl_nstep_return(ptr(rewards), ptr(dones), ptr(values), ptr(last_values),
                                   float(discount), n_env, horizon, promo, ptr(returns),
                                   ptr(advantages), stream_ptr(stream)), "arl_nstep_return")


def valids_mask(reset_flags, n_env, horizon, valids, advantages=None, returns=None, values=None,
                stream=None):
    _want(valids, torch.int8, "valids")
    assert reset_flags.numel() == valids.numel() == n_env * horizon
    _check(load().arl_valids_mask(ptr(reset_flags), n_env, horizon, ptr(valids), ptr(advantages),
                                  ptr(returns), ptr(values), stream_ptr(stream)), "arl_valids_mask")


def standardize_workspace(device):
    return torch.empty(load().arl_standardize_workspace_bytes() // 8, dtype=torch.float64, device=device)


def standardize(advantages, valids, workspace, eps=1e-6, stream=None):
    _want(advantages, torch.float32, "advantages")
    if valids is not None:
        _want(valids, torch.int8, "valids")
        assert valids.numel() == advantages.numel()
    _check(load().arl_standardize(ptr(advantages), ptr(valids), advantages.numel(), float(eps),
                                  ptr(workspace), stream_ptr(stream)), "arl_standardize")


def sample_categorical(prob, uniforms, actions, stream=None):
    _want(prob, torch.float32, "prob")
    _want(uniforms, torch.float64, "uniforms")
    _want(actions, torch.uint8, "actions")
    batch, n_act = prob.shape
    assert uniforms.numel() == batch and actions.numel() == batch
    _check(load().arl_sample_categorical(ptr(prob), ptr(uniforms), batch, n_act, ptr(actions),
                                         stream_ptr(stream)), "arl_sample_categorical")


def preprocess_frames(raw_a, raw_b, out, stream=None, resample="box2x"):
    _want(raw_b, torch.uint8, "raw_b")
    n = raw_b.shape[0]
    assert tuple(raw_b.shape[1:3]) == (RAW_H, RAW_W) and tuple(out.shape) == (n, OBS_H, OBS_W)
    _check(load().arl_preprocess_frames(ptr(raw_a), ptr(raw_b), n, RESAMPLE_MODES[resample], ptr(out),
                                        stream_ptr(stream)), "arl_preprocess_frames")


def gather_scale_obs(obs, idx, out, scale, stream=None):
    _want(obs, torch.uint8, "obs")
    _want(out, torch.float32, "out")
    if idx is not None:
        _want(idx, torch.int32, "idx")
    batch = out.shape[0]
    row_bytes = obs[0].numel()
    assert out[0].numel() == row_bytes and (idx is None or idx.numel() == batch)
    _check(load().arl_gather_scale_obs(ptr(obs), ptr(idx), batch, row_bytes, float(scale), ptr(out),
                                       stream_ptr(stream)), "arl_gather_scale_obs")


def env_act_step(game, state, rollout, prob, value, uniforms, step, mid_batch_reset,
                 max_path_length, discount, active=None, stream=None):
    _check(load().arl_env_act_step(C.byref(game), C.byref(state), C.byref(rollout), ptr(prob),
                                   ptr(value), ptr(uniforms), ptr(active), step,
                                   int(bool(mid_batch_reset)),
                                   float(max_path_length), float(discount), stream_ptr(stream)),
           "arl_env_act_step")


def env_step(game, state, rollout, prob, value, uniforms, step, mid_batch_reset, max_path_length, discount,
             max_start_noops, active=None, single_write=False, stream=None):
    """act_step + frame_step (+ epoch bump) as ONE launch."""
    _check(load().arl_env_step(C.byref(game), C.byref(state), C.byref(rollout), ptr(prob), ptr(value),
                               ptr(uniforms), ptr(active), step, int(bool(mid_batch_reset)),
                               float(max_path_length), float(discount), int(max_start_noops),
                               int(bool(single_write)), stream_ptr(stream)), "arl_env_step")


def serve_conv1_supported(game, geom):
    """Can arl_env_step_served evaluate this first convolution inside its launch?"""
    return bool(load().arl_serve_conv1_supported(C.byref(game), C.byref(geom)))


def rollout_begin_conv1(game, state, rollout, conv1, stream=None):
    """rollout_begin + the first convolution of the rows it copies (conv1: ArlServeConv1), one launch."""
    _check(load().arl_rollout_begin_conv1(C.byref(game), C.byref(state), C.byref(rollout), C.byref(conv1),
                                          stream_ptr(stream)), "arl_rollout_begin_conv1")


def env_step_served(game, state, rollout, head, conv1, uniforms, step, max_path_length, discount, max_start_noops,
                    stream=None):
    """Hidden-layer fold + heads + softmax + action draw + env step (+ the next observation's conv 1) as ONE launch.
    head: ArlServeHead; conv1: ArlServeConv1 or None.  Both hold raw pointers: the caller keeps the tensors alive."""
    _want(uniforms, torch.float64, "uniforms")
    _check(load().arl_env_step_served(C.byref(game), C.byref(state), C.byref(rollout), C.byref(head),
                                      None if conv1 is None else C.byref(conv1), ptr(uniforms), int(step),
                                      float(max_path_length), float(discount), int(max_start_noops),
                                      stream_ptr(stream)), "arl_env_step_served")


def env_frame_step(game, state, rollout, step, max_start_noops, stream=None):
    _check(load().arl_env_frame_step(C.byref(game), C.byref(state), C.byref(rollout), step,
                                     int(max_start_noops), stream_ptr(stream)), "arl_env_frame_step")


def rollout_begin(game, state, rollout, stream=None):
    """observations[:, 0] = step_obs and done_count = 0, one launch."""
    _check(load().arl_rollout_begin(C.byref(game), C.byref(state), C.byref(rollout), stream_ptr(stream)),
           "arl_rollout_begin")


def env_reset(game, state, rollout, flags, max_start_noops, stream=None):
    _check(load().arl_env_reset(C.byref(game), C.byref(state), C.byref(rollout), ptr(flags),
                                int(max_start_noops), stream_ptr(stream)), "arl_env_reset")


def opt_step(opt, method, learning_rate, avg_factor, clip, beta1_or_rho, beta2, epsilon, stream=None):
    _check(load().arl_opt_step(C.byref(opt), method, learning_rate, avg_factor,
                               0.0 if clip is None else clip, beta1_or_rho, beta2, epsilon,
                               stream_ptr(stream)), "arl_opt_step")


OPT_NORM_SLOTS, OPT_NORM_BLOCKS = 64, 2048


def opt_step_noclip(opt, method, learning_rate, avg_factor, beta1_or_rho, beta2, epsilon, k, step_pp, norm_parts,
                    stream=None):
    _check(load().arl_opt_step_noclip(C.byref(opt), method, learning_rate, avg_factor, beta1_or_rho, beta2, epsilon,
                                      int(k), ptr(step_pp), ptr(norm_parts), stream_ptr(stream)), "arl_opt_step_noclip")


def opt_finish(opt, n_updates, avg_factor, step_pp, norm_parts, stream=None, hole_count=0):
    """Close a call of no-clip updates; hole_count: the call's updates were split around a hole of that size."""
    _check(load().arl_opt_finish_split(C.byref(opt), int(n_updates), avg_factor, ptr(step_pp), ptr(norm_parts),
                                       int(hole_count), stream_ptr(stream)), "arl_opt_finish_split")


def opt_step_noclip_split(opt, method, learning_rate, avg_factor, beta1_or_rho, beta2, epsilon, k, step_pp,
                          norm_parts, hole_first, hole_count, part, stream=None):
    """part 0: the no-clip update of everything but [hole_first, hole_first + hole_count); part 1: of that range."""
    _check(load().arl_opt_step_noclip_split(C.byref(opt), method, learning_rate, avg_factor, beta1_or_rho, beta2,
                                            epsilon, int(k), ptr(step_pp), ptr(norm_parts), int(hole_first),
                                            int(hole_count), int(part), stream_ptr(stream)),
           "arl_opt_step_noclip_split")


def corun_job(opt, method, learning_rate, avg_factor, beta1_or_rho, beta2, epsilon, k, step_pp, norm_parts,
              hole_first, hole_count):
    """Part 1 of update k (the hole) as a job for a data-gradient launch to carry (arl_corun_job): plain data, held
    by the caller; conv2d_bwd_data / FoldList.conv2d_bwd_pair take it through `corun=`, corun_job_run runs it alone."""
    job = ArlCorunJob()
    _check(load().arl_corun_job_init(C.byref(job), C.byref(opt), method, learning_rate, avg_factor, beta1_or_rho, beta2,
                                     epsilon, int(k), ptr(step_pp), ptr(norm_parts), int(hole_first), int(hole_count)),
           "arl_corun_job_init")
    return job


def corun_job_run(job, stream=None):
    _check(load().arl_corun_job_run(C.byref(job), stream_ptr(stream)), "arl_corun_job_run")


# ---------------------------------------------------------------------------
# learner glue (csrc/learner.hip)
# ---------------------------------------------------------------------------

def gather_scale_obs_nhwc(obs, idx, out, scale, stream=None):
    """obs u8[n,4,H,W] -> out f32 with NHWC memory ([B,H,W,4] contiguous)."""
    _want(obs, torch.uint8, "obs")
    _want(out, torch.float32, "out")
    if idx is not None:
        _want(idx, torch.int32, "idx")
    batch = out.shape[0]
    channels, plane = obs.shape[1], obs.shape[2] * obs.shape[3]
    assert out.numel() == batch * channels * plane
    _check(load().arl_gather_scale_obs_nhwc(ptr(obs), ptr(idx), batch, channels, plane, float(scale),
                                            out.data_ptr(), stream_ptr(stream)),
           "arl_gather_scale_obs_nhwc")


def traj_minibatch(seg, horizon, state_in, valids, idx, state_out, inv_count=None, stream=None):
    """One launch (arl_traj_minibatch): idx <- the rows of segments `seg` in time order, state_out[s] <- the rows of
    state_in[s] stored before step 0 of each chosen segment, inv_count <- 1 / (valid rows of the minibatch).
    seg i32[n_seg]; state_in: f32 [n_traj * horizon][H] tensors (0 .. 2 of them); valids i8 [n_traj * horizon] or
    None; idx i32[n_seg * horizon]; state_out: f32 [n_seg][H] tensors.  The caller guarantees seg < n_traj."""
    _want(seg, torch.int32, "seg")
    _want(idx, torch.int32, "idx")
    n_seg, n_state = seg.numel(), len(state_in)
    if len(state_out) != n_state:
        raise ValueError("traj_minibatch: %d states in, %d out" % (n_state, len(state_out)))
    if idx.numel() != n_seg * horizon:
        raise ValueError("traj_minibatch: idx holds %d rows, not %d segments x %d" % (idx.numel(), n_seg, horizon))
    hidden, total = 0, None
    for a, b in zip(state_in, state_out):
        _want(a, torch.float32, "state_in")
        _want(b, torch.float32, "state_out")
        hidden = a.shape[-1]
        if b.numel() != n_seg * hidden or a.numel() % (hidden * horizon) or total not in (None, a.numel() // hidden):
            raise ValueError("traj_minibatch: state shapes %s -> %s" % (tuple(a.shape), tuple(b.shape)))
        total = a.numel() // hidden
    if valids is not None:
        _want(valids, torch.int8, "valids")
        if valids.numel() % horizon or total not in (None, valids.numel()):
            raise ValueError("traj_minibatch: valids holds %d rows" % valids.numel())
        total = valids.numel()
    if inv_count is not None:
        _want(inv_count, torch.float32, "inv_count")
    n_traj = (total // horizon) if total is not None else 2 ** 31 // max(horizon, 1) - 1       # (nothing indexed by it)
    arr = C.c_void_p * max(n_state, 1)
    sin, sout = arr(*[ptr(a) for a in state_in]), arr(*[ptr(b) for b in state_out])
    _check(load().arl_traj_minibatch(ptr(seg), n_seg, horizon, n_traj, sin, n_state, hidden, ptr(valids), ptr(idx), sout,
                                     ptr(inv_count), stream_ptr(stream)), "arl_traj_minibatch")


def bias_relu(x, bias, rows, channels, stream=None):
    _check(load().arl_bias_relu(x.data_ptr(), bias.data_ptr(), rows, channels, stream_ptr(stream)),
           "arl_bias_relu")


def relu_bwd_workspace(device):
    return torch.empty(load().arl_relu_bwd_workspace_bytes() // 4, dtype=torch.float32, device=device)


def relu_bwd_bias_grad(dy, y, rows, channels, dbias, workspace, stream=None):
    _check(load().arl_relu_bwd_bias_grad(dy.data_ptr(), y.data_ptr(), rows, channels,
                                         dbias.data_ptr(), ptr(workspace), stream_ptr(stream)),
           "arl_relu_bwd_bias_grad")


def pg_head_workspace(device):
    return torch.zeros(load().arl_pg_head_workspace_bytes() // 4, dtype=torch.float32, device=device)


def pg_head_infer(h, w_head, b_head, prob, value, stream=None):
    batch, hid = h.shape
    n_act = prob.shape[1]
    _check(load().arl_pg_head_infer(ptr(h), w_head.data_ptr(), b_head.data_ptr(), batch, hid, n_act,
                                    ptr(prob), ptr(value), stream_ptr(stream)), "arl_pg_head_infer")


def pg_head_loss(h, w_head, b_head, actions, advantages, returns, old_prob, valids, idx, lr_mult,
                 inv_count, n_actions, kind, clip_param, v_loss_coeff, ent_loss_coeff,
                 dout, dh, dw_head, db_head, loss4, workspace, stream=None, relu_mask_dh=False,
                 tie_rule=PPO_TIE_THEANO):
    """relu_mask_dh: h is a rectifier's output; return dh already multiplied by (h > 0)."""
    batch, hid = h.shape
    _check(load().arl_pg_head_loss(
        ptr(h), w_head.data_ptr(), b_head.data_ptr(), ptr(actions), ptr(advantages), ptr(returns),
        ptr(old_prob), ptr(valids), ptr(idx), ptr(lr_mult), ptr(inv_count), batch, hid, n_actions,
        kind, int(tie_rule), float(clip_param), float(v_loss_coeff), float(ent_loss_coeff), int(bool(relu_mask_dh)), ptr(dout), ptr(dh),
        dw_head.data_ptr(), db_head.data_ptr(), ptr(loss4), ptr(workspace), stream_ptr(stream)),
        "arl_pg_head_loss")


# ---------------------------------------------------------------------------
# fp32 MFMA contractions (csrc/mfma_conv.hip); activations NHWC, weights (K, kh, kw, C)
# ---------------------------------------------------------------------------

def conv_geom(batch, in_h, in_w, in_c, out_c, kh, kw, stride, pad_h, pad_w, route=None):
    return ArlConvGeom(batch, in_h, in_w, in_c, out_c, kh, kw, stride, pad_h, pad_w,
                       default_route if route is None else route)


def dense_geom(batch, fan_in, units, route=None):
    return ArlConvGeom(batch, 1, 1, fan_in, units, 1, 1, 1, 0, 0, default_route if route is None else route)


def with_route(geom, route=None):
    """A copy of geom on another route (default: this module's current default)."""
    g = ArlConvGeom.from_buffer_copy(geom)
    g.route = default_route if route is None else route
    return g


# arl_dev_conv_launch_log (include/accel_rl_hip_dev.h: ARL_DEV_K_*, ARL_DEV_F_*, ARL_DEV_LAUNCH_LOG_MAX)
DEV_LAUNCH_FAMILIES = (None, "igemm", "igemm_occ", "igemm_split", "igemm_u8", "rowgather", "wgrad", "wgrad_fast",
                       "wgrad_split", "wgrad_u8", "bwd_pair", "wgrad_group", "conv1_img", "fold", "fold_many",
                       "dgrad_weights")
DEV_LAUNCH_FLAGS = ("b_kc", "n16", "u8", "multi_tap", "has_pad", "direct", "corun", "tap_uniform")
DEV_LAUNCH_LOG_MAX = 32
ConvLaunch = collections.namedtuple("ConvLaunch", "family tile minw flags split_mode splits grid lds_bytes")


def conv_launch_log():
    """The launches of this thread's most recent conv / dense entry-point call, in issue order: ConvLaunch(family name,
    (WGM, WGN, TM, TN, BK), minw, frozenset of flag names, split mode, splits, (x, y, z), dynamic LDS bytes)."""
    rec = (ArlDevLaunch * DEV_LAUNCH_LOG_MAX)()
    n = load().arl_dev_conv_launch_log(rec, DEV_LAUNCH_LOG_MAX)
    if n > DEV_LAUNCH_LOG_MAX:
        raise RuntimeError("conv launch log: %d launches, only %d kept" % (n, DEV_LAUNCH_LOG_MAX))
    return [ConvLaunch(DEV_LAUNCH_FAMILIES[r.family], (r.wgm, r.wgn, r.tm, r.tn, r.bk), r.minw,
                       frozenset(f for i, f in enumerate(DEV_LAUNCH_FLAGS) if r.flags >> i & 1), r.split_mode, r.splits,
                       (r.grid_x, r.grid_y, r.grid_z), r.lds_bytes) for r in rec[:n]]


def conv_out_hw(g):
    return ((g.in_h + 2 * g.pad_h - g.kh) // g.stride + 1, (g.in_w + 2 * g.pad_w - g.kw) // g.stride + 1)


def conv_workspace(device):
    return torch.empty(load().arl_conv_workspace_bytes() // 4, dtype=torch.float32, device=device)


def relu_bits_shape(rows, channels):
    """Shape of the i32 tensor that holds an f32[rows][channels] activation's rectifier mask as bits (32 channels per
    word, bit c % 32 of word c // 32 = y[row][c] > 0; accel_rl_hip.h: y_bits_or_null)."""
    assert channels % 32 == 0, "rectifier bits need a multiple of 32 channels"
    return (rows, channels // 32)


def _want_bits(bits, n_values, name):
    """A rectifier-bits tensor for n_values activations (None passes).  Its channel count and alignment are the library's
    to check: it refuses, with its own error codes, what it cannot serve."""
    if bits is not None:
        _want(bits, torch.int32, name)
        assert bits.numel() * 32 >= n_values, name + " size"


def _conv2d_fwd(x, w, bias, y, y_bits, geom, relu, workspace, item, stream):
    for t, n in ((x, "x"), (w, "w"), (y, "y")):
        _want(t, torch.float32, n)
    ho, wo = conv_out_hw(geom)
    assert x.numel() == geom.batch * geom.in_h * geom.in_w * geom.in_c, "x size"
    assert w.numel() == geom.out_c * geom.kh * geom.kw * geom.in_c, "w size"
    assert y.numel() == geom.batch * ho * wo * geom.out_c, "y size"
    _want_bits(y_bits, y.numel(), "y_bits")
    _check(load().arl_conv2d_fwd(x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(), ptr(y_bits), C.byref(geom),
                                 int(bool(relu)), ptr(workspace), item, stream_ptr(stream)), "arl_conv2d_fwd")


def conv2d_fwd(x, w, bias, y, geom, relu, workspace, stream=None, y_bits=None):
    """y[B,Ho,Wo,K] = act(conv(x[B,H,W,C], w[K,kh,kw,C]) + bias); all fp32 contiguous memory.
    y_bits (i32, relu_bits_shape): the launch also writes y's rectifier mask as bits."""
    _conv2d_fwd(x, w, bias, y, y_bits, geom, relu, workspace, None, stream)


def conv2d_fwd_parts(x, w, bias, y, geom, relu, workspace, stream=None):
    """conv2d_fwd that leaves a split reduction unfolded: returns the ArlFoldItem describing the partial sums in
    `workspace` (splits == 0: the launch did not split and y is final, bias / rectifier applied)."""
    item = ArlFoldItem()
    _conv2d_fwd(x, w, bias, y, None, geom, relu, workspace, C.byref(item), stream)
    return item


def conv2d_fwd_plan(geom):
    """(splits, k_per_split) of conv2d_fwd on this geometry (arl_conv2d_fwd_plan; nothing is launched)."""
    splits, per = _i32(), _i32()
    _check(load().arl_conv2d_fwd_plan(C.byref(geom), C.byref(splits), C.byref(per)), "arl_conv2d_fwd_plan")
    return splits.value, per.value


def conv2d_u8_supported(in_h, in_w, out_c, kh, kw, stride, pad_h, pad_w):
    """Geometries arl_conv2d_u8_fwd / _bwd_weight_parts accept (see include/accel_rl_hip.h)."""
    return (pad_h == 0 and pad_w == 0 and stride % 4 == 0 and in_w % 4 == 0 and (in_h * in_w) % 4 == 0 and
            kw in (4, 8, 16) and kh % (16 // kw) == 0 and out_c % 4 == 0 and out_c <= 32)


def _u8_rows(obs, idx, geom):
    _want(obs, torch.uint8, "obs")
    assert obs.is_contiguous() and obs.numel() == obs.shape[0] * geom.in_c * geom.in_h * geom.in_w, "obs shape"
    if idx is not None:
        _want(idx, torch.int32, "idx")
        assert idx.numel() == geom.batch, "idx length"
    else:
        assert obs.shape[0] == geom.batch, "obs rows"


def conv2d_u8_fwd(obs, idx, scale, w, bias, y, geom, relu, stream=None, y_bits=None):
    """y[B,Ho,Wo,K] = act(conv(float(obs[idx]) * scale, w[K,C,kh,kw]) + bias), obs u8[n,C,H,W] read in place.
    y_bits: as conv2d_fwd."""
    _u8_rows(obs, idx, geom)
    ho, wo = conv_out_hw(geom)
    assert w.numel() == geom.out_c * geom.kh * geom.kw * geom.in_c, "w size"
    assert y.numel() == geom.batch * ho * wo * geom.out_c, "y size"
    _want_bits(y_bits, y.numel(), "y_bits")
    _check(load().arl_conv2d_u8_fwd(obs.data_ptr(), obs.shape[0], ptr(idx), float(scale), w.data_ptr(), ptr(bias),
                                    y.data_ptr(), ptr(y_bits), C.byref(geom), int(bool(relu)), stream_ptr(stream)),
           "arl_conv2d_u8_fwd")


def conv2d_dgrad_weights(layers, stream=None):
    """layers: [(w, wt, geom)] -- wt <- the data gradient's k-contiguous copy of w (arl_conv2d_dgrad_weights), one launch."""
    assert 0 < len(layers) <= DGRAD_WT_MAX
    items = (ArlDgradWt * len(layers))()
    for it, (w, wt, geom) in zip(items, layers):
        _want(w, torch.float32, "w")
        _want(wt, torch.float32, "wt")
        assert w.numel() == wt.numel() == geom.out_c * geom.kh * geom.kw * geom.in_c, "w / wt size"
        it.w, it.wt, it.geom = ptr(w), ptr(wt), C.pointer(geom)
    _check(load().arl_conv2d_dgrad_weights(items, len(layers), stream_ptr(stream)), "arl_conv2d_dgrad_weights")


def conv2d_bwd_data(dy, w, mask, dx, geom, stream=None, corun=None, wt=None, mask_bits=None):
    """corun: an ArlCorunJob the launch may carry; returns True if it did (else the caller runs it: corun_job_run).
    wt: conv2d_dgrad_weights' copy of w (same results; the split kernels read it instead of w).
    mask_bits: the mask's rectifier bits from the forward's y_bits (same results; read instead of the floats)."""
    ho, wo = conv_out_hw(geom)
    assert dy.numel() == geom.batch * ho * wo * geom.out_c, "dy size"
    assert dx.numel() == geom.batch * geom.in_h * geom.in_w * geom.in_c, "dx size"
    assert mask is None or mask.numel() == dx.numel()
    taken = _i32(0)
    _want_bits(mask_bits, dx.numel(), "mask_bits")
    _check(load().arl_conv2d_bwd_data(dy.data_ptr(), w.data_ptr(), ptr(wt), ptr(mask), ptr(mask_bits), dx.data_ptr(),
                                      C.byref(geom), None if corun is None else C.byref(corun), C.byref(taken),
                                      stream_ptr(stream)), "arl_conv2d_bwd_data")
    return bool(taken.value)


def conv2d_bwd_weight(dy, x, dw, geom, workspace, stream=None):
    ho, wo = conv_out_hw(geom)
    assert dy.numel() == geom.batch * ho * wo * geom.out_c, "dy size"
    assert x.numel() == geom.batch * geom.in_h * geom.in_w * geom.in_c, "x size"
    assert dw.numel() == geom.out_c * geom.kh * geom.kw * geom.in_c, "dw size"
    _check(load().arl_conv2d_bwd_weight(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), C.byref(geom),
                                        ptr(workspace), stream_ptr(stream)), "arl_conv2d_bwd_weight")


class FoldList(object):
    """Pending split folds of one backward pass (arl_fold_item): the *_parts calls append, run()
    folds everything in one launch.  Every appended call needs its own workspace tensor.
    With defer=True a weight-gradient call only plans its launch (arl_wgrad_plan; its fold items are appended as
    usual): run_wgrads() then issues the planned ones, the group-eligible in one launch (arl_conv2d_bwd_weight_group),
    before run()."""

    def __init__(self):
        self._items = (ArlFoldItem * FOLD_MAX_ITEMS)()
        self._n = 0
        self._plans = (ArlWgradPlan * WGRAD_GROUP_MAX)()
        self._n_plans = 0
        self.last_dw_in_place = False
        self.corun_taken = False

    def _next(self):
        assert self._n < FOLD_MAX_ITEMS, "too many pending folds"
        self._n += 1
        return C.byref(self._items[self._n - 1])

    def _bias_slot(self, dbias):
        """(dbias pointer, item pointer) for the optional bias-gradient partials of a weight-gradient call."""
        if dbias is None:
            return None, None
        return dbias.data_ptr(), self._next()

    def _bias_done(self, dbias):
        """False when the kernel could not produce the bias partials (generic path): drop the slot."""
        if dbias is None:
            return True
        if self._items[self._n - 1].splits < 0:
            self._n -= 1
            return False
        return True

    def _next_plan(self, stream):
        if self._n_plans == WGRAD_GROUP_MAX:        # a full list goes out as a group of its own
            self.run_wgrads(stream)
        self._n_plans += 1
        return C.byref(self._plans[self._n_plans - 1])

    def run_wgrads(self, stream=None):
        """The deferred weight gradients' launch(es); their folds stay pending."""
        n, self._n_plans = self._n_plans, 0
        if n:
            _check(load().arl_conv2d_bwd_weight_group(self._plans, n, stream_ptr(stream)), "arl_conv2d_bwd_weight_group")

    def conv2d_bwd_weight(self, dy, x, dw, geom, workspace, dbias=None, stream=None, defer=False):
        """dw partials (and, with dbias, the column sums of dy) for the deferred fold.  Returns False when
        dbias was asked for but not produced (the caller then uses relu_bwd_bias_grad)."""
        ho, wo = conv_out_hw(geom)
        assert dy.numel() == geom.batch * ho * wo * geom.out_c, "dy size"
        assert x.numel() == geom.batch * geom.in_h * geom.in_w * geom.in_c, "x size"
        assert dw.numel() == geom.out_c * geom.kh * geom.kw * geom.in_c, "dw size"
        item = self._next()
        pb, ib = self._bias_slot(dbias)
        _check(load().arl_conv2d_bwd_weight_parts(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), C.byref(geom),
                                                  ptr(workspace), workspace.numel() * workspace.element_size(),
                                                  item, pb, ib, self._next_plan(stream) if defer else None,
                                                  stream_ptr(stream)), "arl_conv2d_bwd_weight_parts")
        return self._bias_done(dbias)

    def conv2d_u8_bwd_weight(self, dy, obs, idx, scale, dw, geom, workspace, dbias=None, stream=None, defer=False):
        """dw[K,C,kh,kw] partials (and, with dbias, the column sums of dy) of a convolution on u8 observations."""
        _u8_rows(obs, idx, geom)
        ho, wo = conv_out_hw(geom)
        assert dy.numel() == geom.batch * ho * wo * geom.out_c, "dy size"
        assert dw.numel() == geom.out_c * geom.kh * geom.kw * geom.in_c, "dw size"
        item = self._next()
        pb, ib = self._bias_slot(dbias)
        _check(load().arl_conv2d_u8_bwd_weight_parts(dy.data_ptr(), obs.data_ptr(), obs.shape[0], ptr(idx),
                                                     float(scale), dw.data_ptr(), C.byref(geom), ptr(workspace),
                                                     workspace.numel() * workspace.element_size(), item, pb, ib,
                                                     self._next_plan(stream) if defer else None, stream_ptr(stream)),
               "arl_conv2d_u8_bwd_weight_parts")
        return self._bias_done(dbias)

    def conv2d_bwd_pair(self, dy, w, mask, dx, x, dw, geom, workspace, dbias=None, stream=None, corun=None, wt=None,
                        defer=False, mask_bits=None):
        """dx (times mask > 0 if given) and (deferred) dw [+ dbias] of one layer in a single launch.
        mask_bits: as conv2d_bwd_data.
        corun: an ArlCorunJob the data-gradient launch may carry; `self.corun_taken` says whether it did.
        wt: conv2d_dgrad_weights' copy of w for the data gradient.
        defer: a layer that does not pair runs its data gradient now and leaves its weight gradient to run_wgrads()."""
        ho, wo = conv_out_hw(geom)
        assert dy.numel() == geom.batch * ho * wo * geom.out_c, "dy size"
        assert x.numel() == dx.numel() == geom.batch * geom.in_h * geom.in_w * geom.in_c, "x / dx size"
        assert dw.numel() == w.numel() == geom.out_c * geom.kh * geom.kw * geom.in_c, "w / dw size"
        item = self._next()
        slot = self._n - 1
        pb, ib = self._bias_slot(dbias)
        taken = _i32(0)
        _want_bits(mask_bits, dx.numel(), "mask_bits")
        _check(load().arl_conv2d_bwd_pair(dy.data_ptr(), w.data_ptr(), ptr(wt), ptr(mask), ptr(mask_bits), dx.data_ptr(),
                                          x.data_ptr(), dw.data_ptr(), C.byref(geom), ptr(workspace),
                                          workspace.numel() * workspace.element_size(), item, pb, ib,
                                          None if corun is None else C.byref(corun), C.byref(taken),
                                          self._next_plan(stream) if defer else None, stream_ptr(stream)),
               "arl_conv2d_bwd_pair")
        self.corun_taken = bool(taken.value)
        self.last_dw_in_place = self._items[slot].splits == 0      # no split partials: dw is final as written
        return self._bias_done(dbias)

    def relu_bwd_bias_grad(self, dy, y, rows, channels, dbias, workspace, stream=None):
        _check(load().arl_relu_bwd_bias_parts(dy.data_ptr(), y.data_ptr(), rows, channels, dbias.data_ptr(),
                                              ptr(workspace), self._next(), stream_ptr(stream)),
               "arl_relu_bwd_bias_parts")

    def pg_head_loss(self, h, w_head, b_head, actions, advantages, returns, old_prob, valids, idx, lr_mult,
                     inv_count, n_actions, kind, clip_param, v_loss_coeff, ent_loss_coeff,
                     dout, dh, dw_head, db_head, loss4, workspace, stream=None, relu_mask_dh=False,
                 tie_rule=PPO_TIE_THEANO, dgrad_weights=None):
        """pg_head_loss with its three small folds (dw_head, db_head, loss4) left to run().
        dgrad_weights: [(w, wt, geom)] -- the launch also writes these layers' k-contiguous weight copies
        (conv2d_dgrad_weights' work in extra workgroups: one launch less per backward pass)."""
        batch, hid = h.shape
        assert self._n + 3 <= FOLD_MAX_ITEMS, "too many pending folds"
        first = C.byref(self._items[self._n])
        self._n += 3
        wt_items, n_wt = None, 0
        if dgrad_weights:
            n_wt = len(dgrad_weights)
            assert n_wt <= DGRAD_WT_MAX
            wt_items = (ArlDgradWt * n_wt)()
            for it, (w, wt, geom) in zip(wt_items, dgrad_weights):
                it.w, it.wt, it.geom = ptr(w), ptr(wt), C.pointer(geom)
        _check(load().arl_pg_head_loss_parts(
            ptr(h), w_head.data_ptr(), b_head.data_ptr(), ptr(actions), ptr(advantages), ptr(returns),
            ptr(old_prob), ptr(valids), ptr(idx), ptr(lr_mult), ptr(inv_count), batch, hid, n_actions,
            kind, int(tie_rule), float(clip_param), float(v_loss_coeff), float(ent_loss_coeff), int(bool(relu_mask_dh)), ptr(dout),
            ptr(dh), dw_head.data_ptr(), db_head.data_ptr(), ptr(loss4), ptr(workspace), first,
            None if wt_items is None else C.cast(wt_items, _vp), n_wt, stream_ptr(stream)),
            "arl_pg_head_loss_parts")

    def ppg_head_loss(self, h, w_head, b_head, actions, advantages, returns, old_prob, idx, lr_mult, inv_count,
                      n_actions, phase, clip_param, v_loss_coeff, ent_loss_coeff, beta_clone,
                      dout, dh, dw_head, db_head, loss4, workspace, stream=None, relu_mask_dh=False,
                      tie_rule=PPO_TIE_THEANO):
        """PPG's output stage (phase PPG_POLICY / PPG_AUX, csrc/ppg.hip) with its three small folds (dw_head, db_head,
        loss4) left to run(), as pg_head_loss leaves them.  workspace: pg_head_workspace()."""
        batch, hid = h.shape
        assert self._n + 3 <= FOLD_MAX_ITEMS, "too many pending folds"
        first = C.byref(self._items[self._n])
        _check(load().arl_ppg_head_loss_parts(
            ptr(h), ptr(w_head), ptr(b_head), ptr(actions), ptr(advantages), ptr(returns), ptr(old_prob), ptr(idx),
            ptr(lr_mult), ptr(inv_count), batch, hid, n_actions, int(phase), int(tie_rule), float(clip_param),
            float(v_loss_coeff), float(ent_loss_coeff), float(beta_clone), int(bool(relu_mask_dh)), ptr(dout), ptr(dh),
            ptr(dw_head), ptr(db_head), ptr(loss4), ptr(workspace), first, stream_ptr(stream)),
            "arl_ppg_head_loss_parts")
        self._n += 3                # (a refused call leaves no items behind)

    def vmpo_head_loss(self, h, w_head, b_head, actions, psi, returns, old_prob, idx, duals, inv_count, n_actions,
                       v_loss_coeff, dout, dh, dw_head, db_head, loss4, workspace, stream=None, relu_mask_dh=False):
        """V-MPO's output stage (csrc/vmpo.hip: arl_vmpo_head_loss_parts) with its three small folds left to run(), as
        ppg_head_loss leaves them.  psi: vmpo_weights' output; duals: device (eta, alpha).  loss4 = (pi_loss, v_loss,
        mean KL, their plain sum)."""
        batch, hid = h.shape
        assert self._n + 3 <= FOLD_MAX_ITEMS, "too many pending folds"
        first = C.byref(self._items[self._n])
        _check(load().arl_vmpo_head_loss_parts(
            ptr(h), ptr(w_head), ptr(b_head), ptr(actions), ptr(psi), ptr(returns), ptr(old_prob), ptr(idx), ptr(duals),
            ptr(inv_count), batch, hid, n_actions, float(v_loss_coeff), int(bool(relu_mask_dh)), ptr(dout), ptr(dh),
            ptr(dw_head), ptr(db_head), ptr(loss4), ptr(workspace), first, stream_ptr(stream)),
            "arl_vmpo_head_loss_parts")
        self._n += 3                # (a refused call leaves no items behind)

    def ln_relu_bwd(self, dy, y, z, stats, gamma, dy_masked, dz, dgamma, dbeta, workspace, stream=None):
        """ln_relu_bwd with its two column-sum folds (dgamma, dbeta) left to run()."""
        rows, width = _ln_rows(z, gamma, (dy, y, dz), stats)
        assert self._n + 2 <= FOLD_MAX_ITEMS, "too many pending folds"
        first = C.byref(self._items[self._n])
        self._n += 2
        _check(load().arl_ln_relu_bwd(ptr(dy), ptr(y), ptr(z), ptr(stats), ptr(gamma), rows, width, int(bool(dy_masked)),
                                      ptr(dz), ptr(dgamma), ptr(dbeta), ptr(workspace), first, stream_ptr(stream)),
               "arl_ln_relu_bwd")

    def run(self, stream=None):
        self.run_wgrads(stream)                 # (partials that were only planned)
        n, self._n = self._n, 0
        _check(load().arl_fold_many(self._items, n, stream_ptr(stream)), "arl_fold_many")


# ---------------------------------------------------------------------------
# replay memory + sum tree (csrc/replay.hip)
# ---------------------------------------------------------------------------

def replay_append(rb, observations, actions, rewards, dones, horizon, idx, discount, promo=PROMO_NEP50,
                  stream=None):
    _want(observations, torch.uint8, "observations")
    _want(actions, torch.uint8, "actions")
    _want(rewards, torch.float32, "rewards")
    _check(load().arl_replay_append(C.byref(rb), ptr(observations), ptr(actions), ptr(rewards), ptr(dones),
                                    horizon, idx, float(discount), promo, stream_ptr(stream)), "arl_replay_append")


def replay_extract(rb, env_idxs, step_idxs, obs, next_obs, actions, returns, terminals, stream=None):
    _want(env_idxs, torch.int32, "env_idxs")
    _want(step_idxs, torch.int32, "step_idxs")
    _check(load().arl_replay_extract(C.byref(rb), ptr(env_idxs), ptr(step_idxs), env_idxs.numel(), ptr(obs),
                                     ptr(next_obs), ptr(actions), ptr(returns), ptr(terminals),
                                     stream_ptr(stream)), "arl_replay_extract")


def replay_extract_shift(rb, env_idxs, step_idxs, frame_h, frame_w, pad, m_obs, k_next, seed, call, obs, next_obs,
                         actions, returns, terminals, stream=None):
    """replay_extract with DrQ's random shift: obs holds m_obs, next_obs k_next shifted views of every sample, view-major
    (view v of sample j: row v * batch + j).  pad 0: no shift."""
    _want(env_idxs, torch.int32, "env_idxs")
    _want(step_idxs, torch.int32, "step_idxs")
    batch = env_idxs.numel()
    stack = rb.n_stack * rb.frame_bytes
    assert obs.numel() == m_obs * batch * stack and next_obs.numel() == k_next * batch * stack, "obs / next_obs size"
    assert actions.numel() == returns.numel() == terminals.numel() == batch, "actions / returns / terminals size"
    _check(load().arl_replay_extract_shift(C.byref(rb), ptr(env_idxs), ptr(step_idxs), batch, frame_h, frame_w, pad,
                                           m_obs, k_next, int(seed), int(call), ptr(obs), ptr(next_obs), ptr(actions),
                                           ptr(returns), ptr(terminals), stream_ptr(stream)),
           "arl_replay_extract_shift")


def sumtree_find(tree, levels, uniforms, out, stream=None):
    _want(tree, torch.float64, "tree")
    _want(uniforms, torch.float64, "uniforms")
    _want(out, torch.int32, "out")
    _check(load().arl_sumtree_find(ptr(tree), levels, ptr(uniforms), uniforms.numel(), ptr(out),
                                   stream_ptr(stream)), "arl_sumtree_find")


def sumtree_add(tree, levels, idxs, diffs, stream=None):
    _want(tree, torch.float64, "tree")
    _want(idxs, torch.int32, "idxs")
    _want(diffs, torch.float64, "diffs")
    _check(load().arl_sumtree_add(ptr(tree), levels, ptr(idxs), ptr(diffs), idxs.numel(), stream_ptr(stream)),
           "arl_sumtree_add")


def sumtree_sample(tree, levels, uniforms, n, part_size, tree_idxs, env_idxs, step_idxs, probs, n_unique,
                   stream=None):
    _want(tree, torch.float64, "tree"), _want(uniforms, torch.float64, "uniforms")
    _want(tree_idxs, torch.int32, "tree_idxs"), _want(probs, torch.float64, "probs")
    _check(load().arl_sumtree_sample(ptr(tree), levels, ptr(uniforms), uniforms.numel(), n, part_size,
                                     ptr(tree_idxs), ptr(env_idxs), ptr(step_idxs), ptr(probs), ptr(n_unique),
                                     stream_ptr(stream)), "arl_sumtree_sample")


def sumtree_sample_batch(tree, levels, uniforms, n, part_size, tree_idxs, env_idxs, step_idxs, probs, n_unique,
                         beta=0.0, is_weights=None, notify=None, ticket=0, stream=None):
    """sumtree_sample + the batch's importance weights in one launch; uniforms: device or PINNED host f64; notify: a pinned
    int64[1] that receives (ticket << 32) | n_unique when the launch is through (the host polls it)."""
    _want(tree, torch.float64, "tree"), _want(uniforms, torch.float64, "uniforms")
    _want(tree_idxs, torch.int32, "tree_idxs"), _want(probs, torch.float64, "probs")
    if is_weights is not None:
        _want(is_weights, torch.float32, "is_weights")
        assert is_weights.numel() == n
    if notify is not None:
        _want(notify, torch.int64, "notify")
        assert notify.is_pinned()
    _check(load().arl_sumtree_sample_batch(ptr(tree), levels, staged_ptr(uniforms), uniforms.numel(), n, part_size,
                                           ptr(tree_idxs), ptr(env_idxs), ptr(step_idxs), ptr(probs), ptr(n_unique),
                                           float(beta), ptr(is_weights), None if notify is None else notify.data_ptr(),
                                           int(ticket), stream_ptr(stream)), "arl_sumtree_sample_batch")


def sumtree_update_pow(tree, levels, idxs, priorities, last_probs, alpha, stream=None):
    """tree[path of idxs] += f32(priorities ** alpha) - last_probs, one launch (priority_diffs + sumtree_add)."""
    _want(tree, torch.float64, "tree"), _want(idxs, torch.int32, "idxs")
    _want(priorities, torch.float32, "priorities"), _want(last_probs, torch.float64, "last_probs")
    assert priorities.numel() == idxs.numel() == last_probs.numel()
    _check(load().arl_sumtree_update_pow(ptr(tree), levels, ptr(idxs), ptr(priorities), ptr(last_probs), float(alpha),
                                         idxs.numel(), stream_ptr(stream)), "arl_sumtree_update_pow")


def is_weights(probs, beta, out, stream=None):
    _want(probs, torch.float64, "probs"), _want(out, torch.float32, "out")
    _check(load().arl_is_weights(ptr(probs), probs.numel(), float(beta), ptr(out), stream_ptr(stream)),
           "arl_is_weights")


def priority_diffs(priorities, last_probs, alpha, diffs, stream=None):
    _want(priorities, torch.float32, "priorities"), _want(last_probs, torch.float64, "last_probs")
    _check(load().arl_priority_diffs(ptr(priorities), ptr(last_probs), priorities.numel(), float(alpha),
                                     ptr(diffs), stream_ptr(stream)), "arl_priority_diffs")


def sumtree_gather(tree, idxs, out, scale=1.0, stream=None):
    _want(tree, torch.float64, "tree")
    _want(idxs, torch.int32, "idxs")
    _want(out, torch.float64, "out")
    _check(load().arl_sumtree_gather(ptr(tree), ptr(idxs), idxs.numel(), float(scale), ptr(out),
                                     stream_ptr(stream)), "arl_sumtree_gather")


# ---------------------------------------------------------------------------
# categorical DQN output stage (csrc/dqn.hip)
# ---------------------------------------------------------------------------

def catdqn_act(logits, z, override, n_actions, n_atoms, onehot, greedy=None, dueling=False, stream=None):
    batch = onehot.shape[0]
    stride = logits.numel() // (batch * (n_actions + int(dueling)))
    _check(load().arl_catdqn_act(ptr(logits), ptr(z), ptr(override), batch, n_actions, n_atoms, stride,
                                 int(dueling), ptr(onehot), ptr(greedy), stream_ptr(stream)), "arl_catdqn_act")


def catdqn_loss(pred_logits, tgt_next_logits, pol_next_logits, z, actions, returns, terminals, is_weights,
                n_actions, n_atoms, v_min, v_max, gamma_n, dlogits, loss_rows, kl, dueling=False, stream=None):
    batch = actions.numel()
    stride = pred_logits.numel() // (batch * (n_actions + int(dueling)))
    _check(load().arl_catdqn_loss(ptr(pred_logits), ptr(tgt_next_logits), ptr(pol_next_logits), ptr(z),
                                  ptr(actions), ptr(returns), ptr(terminals), ptr(is_weights), batch, n_actions,
                                  n_atoms, stride, int(dueling), float(v_min), float(v_max), float(gamma_n),
                                  ptr(dlogits), ptr(loss_rows), ptr(kl), stream_ptr(stream)), "arl_catdqn_loss")


def logit_src(item, bias, row0=0, row_floats=0):
    """ArlLogitSrc for arl_catdqn_loss_parts from what conv2d_fwd_parts returned for the output layer: rows from `row0`
    on (row_floats floats per row); an unsplit launch (item.splits == 0: `out` is final) reads as one split, no bias."""
    src = ArlLogitSrc()
    split = item.splits > 0
    src.part = (item.part if split else item.out) + 4 * row0 * row_floats
    src.bias_or_null = bias.data_ptr() if (split and bias is not None) else None
    src.split_stride = item.total
    src.splits = item.splits if split else 1
    return src


def catdqn_loss_parts(pred, tgt_next, pol_next, z, actions, returns, terminals, is_weights, n_actions, n_atoms,
                      atom_stride, v_min, v_max, gamma_n, dlogits, loss_rows, kl, dueling=False, stream=None,
                      dgrad_weights=None):
    """arl_catdqn_loss on logit blocks still in split partial sums (ArlLogitSrc each; pol_next None: not double DQN).
    dgrad_weights: [(w, wt, geom)] -- the launch also writes these layers' k-contiguous weight copies."""
    wt_items, n_wt = None, 0
    if dgrad_weights:
        n_wt = len(dgrad_weights)
        assert n_wt <= DGRAD_WT_MAX
        wt_items = (ArlDgradWt * n_wt)()
        for it, (w, wt, geom) in zip(wt_items, dgrad_weights):
            it.w, it.wt, it.geom = ptr(w), ptr(wt), C.pointer(geom)
    _check(load().arl_catdqn_loss_parts(C.byref(pred), C.byref(tgt_next), None if pol_next is None else C.byref(pol_next),
                                        ptr(z), ptr(actions), ptr(returns), ptr(terminals), ptr(is_weights),
                                        actions.numel(), n_actions, n_atoms, atom_stride, int(dueling), float(v_min),
                                        float(v_max), float(gamma_n), ptr(dlogits), ptr(loss_rows), ptr(kl),
                                        None if wt_items is None else C.cast(wt_items, _vp), n_wt,
                                        stream_ptr(stream)), "arl_catdqn_loss_parts")


def qrdqn_act(theta, override, n_actions, n_quantiles, onehot, greedy=None, dueling=False, stream=None):
    batch = onehot.shape[0]
    stride = theta.numel() // (batch * (n_actions + int(dueling)))
    _check(load().arl_qrdqn_act(ptr(theta), ptr(override), batch, n_actions, n_quantiles, stride, int(dueling),
                                ptr(onehot), ptr(greedy), stream_ptr(stream)), "arl_qrdqn_act")


def qrdqn_loss(pred, tgt_next, pol_next, actions, returns, terminals, is_weights, n_actions, n_quantiles, gamma_n, kappa,
               dtheta, loss_rows, priorities, dueling=False, stream=None):
    """kappa 0: plain quantile regression."""
    batch = actions.numel()
    stride = pred.numel() // (batch * (n_actions + int(dueling)))
    _check(load().arl_qrdqn_loss(ptr(pred), ptr(tgt_next), ptr(pol_next), ptr(actions), ptr(returns), ptr(terminals),
                                 ptr(is_weights), batch, n_actions, n_quantiles, stride, int(dueling), float(gamma_n),
                                 float(kappa), ptr(dtheta), ptr(loss_rows), ptr(priorities), stream_ptr(stream)),
           "arl_qrdqn_loss")


# ---- implicit quantile networks (csrc/iqn.hip): theta f32[batch][fractions][a_stride] ----
IQN_COS = 64                    # ARL_IQN_COS
IQN_MAX_FRACTIONS = 64          # ARL_IQN_MAX_FRACTIONS


def iqn_embed(tau_in, state, rows, r, tau, cosf, row0=0, call_offset=0, stream=None):
    """tau f32[rows r] and cosf f32[rows r][64]: given (tau_in) or drawn (state = i64[2] (seed, counter), only read;
    the stream is indexed by the global pair index (row0 + row) r + fraction and by counter + call_offset)."""
    _want(tau, torch.float32, "tau")
    _want(cosf, torch.float32, "cosf")
    assert tau.numel() == rows * r and cosf.numel() == rows * r * IQN_COS, "tau / cosf size"
    if tau_in is not None:
        _want(tau_in, torch.float32, "tau_in")
        assert tau_in.numel() == rows * r, "tau_in size"
    if state is not None:
        _want(state, torch.int64, "state")
    _check(load().arl_iqn_embed(ptr(tau_in), ptr(state), row0, call_offset, rows, r, ptr(tau), ptr(cosf),
                                stream_ptr(stream)), "arl_iqn_embed")


def iqn_merge_fwd(psi, phi, batch, r, f, x, stream=None):
    assert psi.numel() == batch * f and phi.numel() == x.numel() == batch * r * f, "psi / phi / x size"
    _check(load().arl_iqn_merge_fwd(ptr(psi), ptr(phi), batch, r, f, ptr(x), stream_ptr(stream)), "arl_iqn_merge_fwd")


def iqn_merge_bwd(g, psi, phi, batch, r, f, dphi, dpsi, stream=None):
    assert psi.numel() == dpsi.numel() == batch * f, "psi / dpsi size"
    assert g.numel() == phi.numel() == dphi.numel() == batch * r * f, "g / phi / dphi size"
    _check(load().arl_iqn_merge_bwd(ptr(g), ptr(psi), ptr(phi), batch, r, f, ptr(dphi), ptr(dpsi), stream_ptr(stream)),
           "arl_iqn_merge_bwd")


def iqn_act(theta, override, n_actions, k, onehot, greedy=None, state=None, advance=0, stream=None):
    batch = onehot.shape[0]
    stride = theta.numel() // (batch * k)
    _check(load().arl_iqn_act(ptr(theta), ptr(override), batch, n_actions, k, stride, ptr(onehot), ptr(greedy),
                              ptr(state), advance, stream_ptr(stream)), "arl_iqn_act")


def iqn_loss(pred, tau_pred, tgt_next, pol_next, actions, returns, terminals, is_weights, n_actions, n, n_target,
             gamma_n, kappa, dtheta, loss_rows, priorities, state=None, advance=0, stream=None):
    """kappa 0: plain quantile regression.  state: the (seed, counter) buffer to advance by `advance` (drawn fractions)."""
    batch = actions.numel()
    stride = pred.numel() // (batch * n)
    assert tau_pred.numel() == batch * n and tgt_next.numel() == batch * n_target * stride, "tau_pred / tgt_next size"
    assert pol_next is None or pol_next.numel() == tgt_next.numel(), "pol_next size"
    assert dtheta.numel() == pred.numel(), "dtheta size"
    _check(load().arl_iqn_loss(ptr(pred), ptr(tau_pred), ptr(tgt_next), ptr(pol_next), ptr(actions), ptr(returns),
                               ptr(terminals), ptr(is_weights), batch, n_actions, n, n_target, stride, float(gamma_n),
                               float(kappa), ptr(dtheta), ptr(loss_rows), ptr(priorities), ptr(state), advance,
                               stream_ptr(stream)), "arl_iqn_loss")


def miqn_loss(pred, tau_pred, tgt_next, tgt_cur, actions, returns, terminals, is_weights, n_actions, n, n_target,
              gamma_n, kappa, tau_e, alpha, l0, dtheta, loss_rows, priorities, state=None, advance=0, stream=None):
    """Munchausen IQN: tgt_next / tgt_cur are the target net on next_obs / obs; tau_e, alpha, l0 the entropy temperature,
    the bonus scale and the clip floor.  kappa, state and advance as iqn_loss."""
    batch = actions.numel()
    stride = pred.numel() // (batch * n)
    assert tau_pred.numel() == batch * n and tgt_next.numel() == batch * n_target * stride, "tau_pred / tgt_next size"
    assert tgt_cur is None or tgt_cur.numel() == tgt_next.numel(), "tgt_cur size"
    assert dtheta.numel() == pred.numel(), "dtheta size"
    _check(load().arl_miqn_loss(ptr(pred), ptr(tau_pred), ptr(tgt_next), ptr(tgt_cur), ptr(actions), ptr(returns),
                                ptr(terminals), ptr(is_weights), batch, n_actions, n, n_target, stride, float(gamma_n),
                                float(kappa), float(tau_e), float(alpha), float(l0), ptr(dtheta), ptr(loss_rows),
                                ptr(priorities), ptr(state), advance, stream_ptr(stream)), "arl_miqn_loss")


# ---- fully parameterized quantile functions (csrc/fqf.hip): logits f32[batch][n_stride], tau f32[batch][n + 1] ----
def fqf_fractions(logits, n, tau, tau_hat, tau_mid=None, q=None, logq=None, entropy=None, stream=None):
    """Soft-max of the n logits of every row -> tau (n + 1 per row, 0 .. 1), tau_hat (midpoints) and, where given, the
    compact inner fractions tau_mid (n - 1 per row), q, log q and the entropy."""
    batch = tau_hat.numel() // n
    n_stride = logits.numel() // batch
    assert tau.numel() == batch * (n + 1) and tau_hat.numel() == batch * n, "tau / tau_hat size"
    assert tau_mid is None or tau_mid.numel() == batch * (n - 1), "tau_mid size"
    assert all(t is None or t.numel() == batch * n for t in (q, logq)) and (entropy is None or entropy.numel() == batch), \
        "q / logq / entropy size"
    _check(load().arl_fqf_fractions(ptr(logits), batch, n, n_stride, ptr(tau), ptr(tau_hat), ptr(tau_mid), ptr(q),
                                    ptr(logq), ptr(entropy), stream_ptr(stream)), "arl_fqf_fractions")


def fqf_act(theta, tau, override, n_actions, k, onehot, greedy=None, stream=None):
    batch = onehot.shape[0]
    stride = theta.numel() // (batch * k)
    assert tau.numel() == batch * (k + 1), "tau size"
    _check(load().arl_fqf_act(ptr(theta), ptr(tau), ptr(override), batch, n_actions, k, stride, ptr(onehot), ptr(greedy),
                              stream_ptr(stream)), "arl_fqf_act")


def fqf_loss(pred, pred_mid, tau, tau_hat, q, logq, entropy, tgt_next, pol_next, actions, returns, terminals, is_weights,
             n_actions, n, gamma_n, kappa, ent_coef, dtheta, loss_rows, priorities, dlogits, frac_rows, stream=None):
    """pred / tgt_next / pol_next: the nets at tau_hat; pred_mid: the online net at tau_1 .. tau_{n-1} (None when n == 1).
    kappa 0: plain quantile regression.  frac_rows is a surrogate (right gradient, not W1's value)."""
    batch = actions.numel()
    stride = pred.numel() // (batch * n)
    n_stride = dlogits.numel() // batch
    assert tau.numel() == batch * (n + 1) and tau_hat.numel() == q.numel() == logq.numel() == batch * n, "fraction sizes"
    assert tgt_next.numel() == pred.numel() == dtheta.numel() and entropy.numel() == batch, "tgt_next / dtheta / entropy size"
    assert pol_next is None or pol_next.numel() == tgt_next.numel(), "pol_next size"
    assert (pred_mid is None and n == 1) or pred_mid.numel() == batch * (n - 1) * stride, "pred_mid size"
    _check(load().arl_fqf_loss(ptr(pred), ptr(pred_mid), ptr(tau), ptr(tau_hat), ptr(q), ptr(logq), ptr(entropy),
                               ptr(tgt_next), ptr(pol_next), ptr(actions), ptr(returns), ptr(terminals), ptr(is_weights),
                               batch, n_actions, n, stride, n_stride, float(gamma_n), float(kappa), float(ent_coef),
                               ptr(dtheta), ptr(loss_rows), ptr(priorities), ptr(dlogits), ptr(frac_rows),
                               stream_ptr(stream)), "arl_fqf_loss")


def dqn_act(q, override, n_actions, onehot, greedy=None, dueling=False, stream=None):
    batch = onehot.shape[0]
    _check(load().arl_dqn_act(ptr(q), ptr(override), batch, n_actions, q.numel() // batch, int(dueling),
                              ptr(onehot), ptr(greedy), stream_ptr(stream)), "arl_dqn_act")


def dqn_loss(q, tgt_next_q, pol_next_q, actions, returns, terminals, is_weights, n_actions, gamma_n, delta_clip,
             dq, loss_rows, td_abs, dueling=False, stream=None):
    """delta_clip None: squared loss."""
    batch = actions.numel()
    _check(load().arl_dqn_loss(ptr(q), ptr(tgt_next_q), ptr(pol_next_q), ptr(actions), ptr(returns),
                               ptr(terminals), ptr(is_weights), batch, n_actions, q.numel() // batch, int(dueling),
                               float(gamma_n), 0.0 if delta_clip is None else float(delta_clip), ptr(dq),
                               ptr(loss_rows), ptr(td_abs), stream_ptr(stream)), "arl_dqn_loss")


def drq_loss(q, tgt_next_q, pol_next_q, actions, returns, terminals, is_weights, n_actions, gamma_n, delta_clip, m, k,
             dq, loss_rows, td_abs, dueling=False, stream=None):
    """DrQ: q / dq hold m, tgt_next_q / pol_next_q k view-major blocks of `batch` rows.  delta_clip None: squared loss."""
    batch = actions.numel()
    stride = q.numel() // (m * batch)
    assert q.numel() == dq.numel() == m * batch * stride and tgt_next_q.numel() == k * batch * stride, "q / dq / tgt size"
    assert pol_next_q is None or pol_next_q.numel() == tgt_next_q.numel(), "pol_next_q size"
    assert loss_rows.numel() == td_abs.numel() == batch, "loss_rows / td_abs size"
    _check(load().arl_drq_loss(ptr(q), ptr(tgt_next_q), ptr(pol_next_q), ptr(actions), ptr(returns), ptr(terminals),
                               ptr(is_weights), batch, m, k, n_actions, stride, int(dueling), float(gamma_n),
                               0.0 if delta_clip is None else float(delta_clip), ptr(dq), ptr(loss_rows), ptr(td_abs),
                               stream_ptr(stream)), "arl_drq_loss")


def mdqn_loss(q, tgt_next_q, tgt_cur_q, actions, returns, terminals, is_weights, n_actions, gamma_n, delta_clip, tau_e,
              alpha, l0, dq, loss_rows, td_abs, dueling=False, stream=None):
    """Munchausen DQN: tgt_next_q / tgt_cur_q are the target net on next_obs / obs.  delta_clip None: squared loss."""
    batch = actions.numel()
    _check(load().arl_mdqn_loss(ptr(q), ptr(tgt_next_q), ptr(tgt_cur_q), ptr(actions), ptr(returns), ptr(terminals),
                                ptr(is_weights), batch, n_actions, q.numel() // batch, int(dueling), float(gamma_n),
                                0.0 if delta_clip is None else float(delta_clip), float(tau_e), float(alpha), float(l0),
                                ptr(dq), ptr(loss_rows), ptr(td_abs), stream_ptr(stream)), "arl_mdqn_loss")


def sacd_act(logits, override, n_actions, prob, greedy=None, deterministic=False, stream=None):
    """SAC-Discrete serving: the actor's soft-max row, or a one-hot row (deterministic / override)."""
    batch = prob.shape[0]
    _want(logits, torch.float32, "logits")
    assert logits.numel() % batch == 0 and prob.numel() == batch * n_actions, "logits / prob size"
    _check(load().arl_sacd_act(ptr(logits), ptr(override), batch, n_actions, logits.numel() // batch,
                               int(bool(deterministic)), ptr(prob), ptr(greedy), stream_ptr(stream)), "arl_sacd_act")


def sacd_loss(q1, q2, q1t_next, q2t_next, logits, logits_next, actions, returns, terminals, is_weights, log_alpha,
              n_actions, gamma_n, delta_clip, dq1, dq2, dlogits, stats, stream=None):
    """SAC-Discrete: stats f32[4][B] = q_loss_rows | td_abs | pi_loss_rows | ent_rows.  delta_clip None: squared loss."""
    batch = actions.numel()
    n = q1.numel()
    assert n % batch == 0 and all(t.numel() == n for t in (q2, q1t_next, q2t_next, logits, logits_next, dq1, dq2, dlogits)), \
        "the nine row blocks must have one size"
    assert stats.numel() == 4 * batch and log_alpha.numel() >= 1, "stats / log_alpha size"
    _want(log_alpha, torch.float32, "log_alpha")
    _check(load().arl_sacd_loss(ptr(q1), ptr(q2), ptr(q1t_next), ptr(q2t_next), ptr(logits), ptr(logits_next),
                                ptr(actions), ptr(returns), ptr(terminals), ptr(is_weights), ptr(log_alpha), batch,
                                n_actions, n // batch, float(gamma_n), 0.0 if delta_clip is None else float(delta_clip),
                                ptr(dq1), ptr(dq2), ptr(dlogits), ptr(stats), stream_ptr(stream)), "arl_sacd_loss")


def sacd_alpha_grad(ent_rows, log_alpha, target_entropy, grad_out, stream=None):
    """grad_out f32[4]: entry 0 = exp(log_alpha) * (mean(ent_rows) - target_entropy), entries 1 .. 3 = 0."""
    _want(ent_rows, torch.float32, "ent_rows")
    assert grad_out.numel() >= 4 and log_alpha.numel() >= 1, "grad_out / log_alpha size"
    _check(load().arl_sacd_alpha_grad(ptr(ent_rows), ent_rows.numel(), ptr(log_alpha), float(target_entropy),
                                      ptr(grad_out), stream_ptr(stream)), "arl_sacd_alpha_grad")


def q_regress_loss(q, idx, actions, returns, n_actions, delta_clip, dq, loss_rows, td_abs, stream=None):
    """PQN: arl_dqn_loss's TD row against returns[idx] (idx None: row i); delta_clip None: squared loss."""
    batch = loss_rows.numel()
    _want(q, torch.float32, "q")
    _want(actions, torch.uint8, "actions")
    _want(returns, torch.float32, "returns")
    if idx is not None:
        _want(idx, torch.int32, "idx")
        assert idx.numel() == batch, "idx size"
    assert q.numel() == dq.numel() and q.numel() % batch == 0 and td_abs.numel() == batch, "q / dq / td_abs size"
    _check(load().arl_q_regress_loss(ptr(q), ptr(idx), ptr(actions), ptr(returns), batch, n_actions, q.numel() // batch,
                                     0.0 if delta_clip is None else float(delta_clip), ptr(dq), ptr(loss_rows),
                                     ptr(td_abs), stream_ptr(stream)), "arl_q_regress_loss")


def qlambda_scan(q, q_last, rewards, dones, discount, q_lambda, n_env, horizon, n_actions, returns, stream=None):
    """Q(lambda) returns (arl_qlambda_scan): q [n_env * horizon, q_stride], q_last [n_env, q_stride], rows env-major."""
    for t, n in ((q, "q"), (q_last, "q_last"), (rewards, "rewards"), (returns, "returns")):
        _want(t, torch.float32, n)
    _want_flags(dones, "dones")
    stride = q_last.numel() // n_env
    assert q.numel() == n_env * horizon * stride and q_last.numel() == n_env * stride, "q / q_last size"
    assert rewards.numel() == dones.numel() == returns.numel() == n_env * horizon, "rewards / dones / returns size"
    _check(load().arl_qlambda_scan(ptr(q), ptr(q_last), ptr(rewards), ptr(dones), float(discount), float(q_lambda),
                                   n_env, horizon, n_actions, stride, ptr(returns), stream_ptr(stream)),
           "arl_qlambda_scan")


def vtrace_scan(prob, old_prob, actions, values, last_values, rewards, dones, discount, vtrace_lambda, rho_bar, c_bar,
                pg_rho_bar, n_env, horizon, returns, advantages, stats=None, stream=None):
    """V-trace targets and advantages (arl_vtrace_scan): prob, old_prob [n_env * horizon, n_actions], rows env-major;
    stats (optional) f32 [n_env, 2] = (sum of the ratios, steps with ratio > rho_bar) per env."""
    for t, n in ((prob, "prob"), (old_prob, "old_prob"), (values, "values"), (last_values, "last_values"),
                 (rewards, "rewards"), (returns, "returns"), (advantages, "advantages")):
        _want(t, torch.float32, n)
    _want(actions, torch.uint8, "actions")
    _want_flags(dones, "dones")
    steps = n_env * horizon
    n_actions = prob.numel() // steps
    assert prob.numel() == old_prob.numel() == steps * n_actions, "prob / old_prob size"
    assert actions.numel() == values.numel() == rewards.numel() == dones.numel() == steps, "per-step input sizes"
    assert last_values.numel() == n_env and returns.numel() == advantages.numel() == steps, "last_values / output sizes"
    if stats is not None:
        _want(stats, torch.float32, "stats")
        assert stats.numel() == 2 * n_env, "stats size"
    _check(load().arl_vtrace_scan(ptr(prob), ptr(old_prob), ptr(actions), ptr(values), ptr(last_values), ptr(rewards),
                                  ptr(dones), float(discount), float(vtrace_lambda), float(rho_bar), float(c_bar),
                                  float(pg_rho_bar), n_env, horizon, n_actions, ptr(returns), ptr(advantages), ptr(stats),
                                  stream_ptr(stream)), "arl_vtrace_scan")


# ---------------------------------------------------------------------------
# ACER: Retrace scan, head loss, average-network step, segment gather (csrc/acer.hip)
# ---------------------------------------------------------------------------

def acer_retrace_scan(prob, prob_last, q, q_last, old_prob, actions, rewards, dones, discount, retrace_lambda, n_env,
                      horizon, qret, v_out=None, stats=None, stream=None):
    """Retrace(lambda) targets (arl_acer_retrace_scan): prob, old_prob [n_env * horizon, A], prob_last [n_env, A], rows
    env-major; q / q_last are VIEWS of the Q half of the network output (rows [.., q_stride], the first A columns read):
    their row stride is taken from the tensors.  stats (optional) f32 [n_env, 2] = (sum of rho, steps with rho > 1)."""
    for t, n in ((prob, "prob"), (prob_last, "prob_last"), (q, "q"), (q_last, "q_last"), (old_prob, "old_prob"),
                 (rewards, "rewards"), (qret, "qret"), (v_out, "v_out"), (stats, "stats")):
        if t is not None:
            _want(t, torch.float32, n)
    _want(actions, torch.uint8, "actions")
    _want_flags(dones, "dones")
    steps = n_env * horizon
    n_actions = prob_last.numel() // n_env
    assert prob.numel() == old_prob.numel() == steps * n_actions and prob_last.numel() == n_env * n_actions, "prob sizes"
    assert actions.numel() == rewards.numel() == dones.numel() == qret.numel() == steps, "per-step sizes"
    assert v_out is None or v_out.numel() == steps, "v_out size"
    assert stats is None or stats.numel() == 2 * n_env, "stats size"
    for t, rows in ((q, steps), (q_last, n_env)):
        if not (t.dim() == 2 and t.shape[0] == rows and t.shape[1] >= n_actions and t.stride(1) == 1 and t.is_cuda):
            raise ValueError("q / q_last: device rows [%d, >= %d] with unit column stride" % (rows, n_actions))
    stride = q.stride(0)                        # (a one-row view keeps the stride of the block it was cut from)
    if n_env > 1 and q_last.stride(0) != stride:
        raise ValueError("q and q_last must share one row stride")
    _check(load().arl_acer_retrace_scan(ptr(prob), ptr(prob_last), q.data_ptr(), q_last.data_ptr(), stride,
                                        ptr(old_prob), ptr(actions), ptr(rewards), ptr(dones), float(discount),
                                        float(retrace_lambda), n_env, horizon, n_actions, ptr(qret), ptr(v_out),
                                        ptr(stats), stream_ptr(stream)), "arl_acer_retrace_scan")


def acer_loss(out, out_avg, old_prob, actions, qret, idx, n_actions, c, delta, q_coeff, ent_coeff, dout, stats,
              stream=None):
    """ACER's output stage (arl_acer_loss): out, out_avg, dout f32 [B, 2S]; old_prob / actions / qret full-batch arrays
    read at idx (None: row b); stats f32 [5, B] = pi_loss_rows | q_loss_rows | ent_rows | trust scale | rho(a_t)."""
    batch = stats.numel() // 5
    for t, n in ((out, "out"), (out_avg, "out_avg"), (old_prob, "old_prob"), (qret, "qret"), (dout, "dout"),
                 (stats, "stats")):
        _want(t, torch.float32, n)
    _want(actions, torch.uint8, "actions")
    if idx is not None:
        _want(idx, torch.int32, "idx")
        assert idx.numel() == batch, "idx size"
    assert stats.numel() == 5 * batch and out.numel() == out_avg.numel() == dout.numel() and \
        out.numel() % (2 * batch) == 0, "out / out_avg / dout / stats size"
    _check(load().arl_acer_loss(ptr(out), ptr(out_avg), ptr(old_prob), ptr(actions), ptr(qret), ptr(idx), batch,
                                n_actions, out.numel() // (2 * batch), float(c), float(delta), float(q_coeff),
                                float(ent_coeff), ptr(dout), ptr(stats), stream_ptr(stream)), "arl_acer_loss")


def acer_avg_step(avg, params, alpha, stream=None):
    """avg <- alpha avg + (1 - alpha) params (arl_acer_avg_step), fp32, no fma."""
    _want(avg, torch.float32, "avg")
    _want(params, torch.float32, "params")
    assert avg.numel() == params.numel(), "avg / params size"
    _check(load().arl_acer_avg_step(ptr(avg), ptr(params), avg.numel(), float(alpha), stream_ptr(stream)),
           "arl_acer_avg_step")


def gather_segments(src, index, dst, stream=None):
    """dst[i] = src[index[i]] over the leading axis (arl_gather_segments): index i32 on the device, clamped into range."""
    _want(index, torch.int32, "index")
    n_seg, n_src = dst.shape[0], src.shape[0]
    if src.dtype != dst.dtype or tuple(src.shape[1:]) != tuple(dst.shape[1:]) or index.numel() != n_seg:
        raise ValueError("gather_segments: src %s %s, dst %s %s, index of %d" %
                         (tuple(src.shape), src.dtype, tuple(dst.shape), dst.dtype, index.numel()))
    seg_bytes = src[0].numel() * src.element_size()
    _check(load().arl_gather_segments(ptr(src), ptr(index), n_seg, n_src, seg_bytes, ptr(dst), stream_ptr(stream)),
           "arl_gather_segments")


# ---------------------------------------------------------------------------
# V-MPO: top-half weights and the duals' step (csrc/vmpo.hip; the head's loss is FoldList.vmpo_head_loss)
# ---------------------------------------------------------------------------

def vmpo_weights(advantages, idx, duals, eps_eta, psi, temp4, stream=None):
    """psi[rows of the minibatch] = softmax(A / eta) over the top half of its advantages, 0 on its other rows (rows
    outside it are left alone); temp4 = (temp_loss, d temp_loss / d eta, log mean exp(A / eta), n_top).  idx None: the
    minibatch is rows 0 .. psi.numel() - 1.  duals: device f32[2] = (eta, alpha)."""
    for t, n in ((advantages, "advantages"), (duals, "duals"), (psi, "psi"), (temp4, "temp4")):
        _want(t, torch.float32, n)
    if idx is not None:
        _want(idx, torch.int32, "idx")
    assert psi.numel() == advantages.numel() and duals.numel() >= 2 and temp4.numel() >= 4, "psi / duals / temp4 size"
    n = advantages.numel() if idx is None else idx.numel()
    assert n <= advantages.numel(), "more positions than rows"
    _check(load().arl_vmpo_weights(ptr(advantages), ptr(idx), n, ptr(duals), float(eps_eta), ptr(psi), ptr(temp4),
                                   stream_ptr(stream)), "arl_vmpo_weights")


def vmpo_dual_step(duals, slot0, slot1, step_count, lr_mult, temp4, loss4, eps_alpha, method, learning_rate,
                   beta1_or_rho, beta2, epsilon, stream=None):
    """One optimiser step on (eta, alpha) from (temp4[1], eps_alpha - loss4[2]), then max(x, 1e-8); step_count += 1."""
    for t, n in ((duals, "duals"), (slot0, "slot0"), (step_count, "step_count"), (lr_mult, "lr_mult"), (temp4, "temp4"),
                 (loss4, "loss4")):
        _want(t, torch.float32, n)
    assert duals.numel() >= 2 and slot0.numel() >= 2 and (slot1 is None or slot1.numel() >= 2), "duals / slot sizes"
    assert temp4.numel() >= 4 and loss4.numel() >= 4, "temp4 / loss4 size"
    _check(load().arl_vmpo_dual_step(ptr(duals), ptr(slot0), ptr(slot1), ptr(step_count), ptr(lr_mult), ptr(temp4),
                                     ptr(loss4), float(eps_alpha), int(method), float(learning_rate), float(beta1_or_rho),
                                     float(beta2), float(epsilon), stream_ptr(stream)), "arl_vmpo_dual_step")


# ---------------------------------------------------------------------------
# RND: observation statistics, network input, prediction error, reward mix (csrc/rnd.hip)
# ---------------------------------------------------------------------------

def _rnd_frames(observations, extra_observations, n_env, horizon):
    _want(observations, torch.uint8, "observations")
    _want(extra_observations, torch.uint8, "extra_observations")
    c, h, w = (int(s) for s in observations.shape[1:])
    assert observations.shape[0] == n_env * horizon and tuple(extra_observations.shape) == (n_env, c, h, w), \
        "observations [n_env * horizon, C, H, W] and extra_observations [n_env, C, H, W]"
    return c, h, w


def rnd_obs_stats_workspace(h, w, device):
    return torch.empty(load().arl_rnd_obs_stats_workspace_bytes(h, w) // 8, dtype=torch.float64, device=device)


def rnd_obs_stats(observations, extra_observations, n_env, horizon, count, mean, m2, workspace, stream=None):
    """Chan-merge the per-pixel moments of the batch's next-observation frames (newest plane) into (count, mean, m2)."""
    c, h, w = _rnd_frames(observations, extra_observations, n_env, horizon)
    for t, n in ((count, "count"), (mean, "mean"), (m2, "m2"), (workspace, "workspace")):
        _want(t, torch.float64, n)
    assert count.numel() == 1 and mean.numel() == m2.numel() == h * w, "count f64[1], mean and m2 f64[H * W]"
    assert workspace.numel() * 8 >= load().arl_rnd_obs_stats_workspace_bytes(h, w), "workspace too small"
    _check(load().arl_rnd_obs_stats(ptr(observations), ptr(extra_observations), n_env, horizon, c, h, w, ptr(count),
                                    ptr(mean), ptr(m2), ptr(workspace), stream_ptr(stream)), "arl_rnd_obs_stats")


def rnd_obs_prepare(observations, extra_observations, idx, n_env, horizon, count, mean, m2, out, stream=None):
    """out f32[B, H, W, 4]: channel 0 = the normalised, clamped next-observation frame of rows idx (None: rows 0 .. B - 1)."""
    c, h, w = _rnd_frames(observations, extra_observations, n_env, horizon)
    for t, n in ((count, "count"), (mean, "mean"), (m2, "m2")):
        _want(t, torch.float64, n)
    _want(out, torch.float32, "out")
    if idx is not None:
        _want(idx, torch.int32, "idx")
    batch = out.shape[0]
    assert count.numel() == 1 and mean.numel() == m2.numel() == h * w, "count f64[1], mean and m2 f64[H * W]"
    assert out.numel() == batch * h * w * 4 and (idx is None or idx.numel() == batch), "out [B, H, W, 4], idx [B]"
    _check(load().arl_rnd_obs_prepare(ptr(observations), ptr(extra_observations), ptr(idx), batch, n_env, horizon, c, h, w,
                                      ptr(count), ptr(mean), ptr(m2), ptr(out), stream_ptr(stream)),
           "arl_rnd_obs_prepare")


def rnd_error(pred, targ, err, dpred=None, loss=None, stream=None):
    """err[b] = mean_e (pred - targ)^2; with dpred and loss also its gradient for the mean over rows, and that mean."""
    for t, n in ((pred, "pred"), (targ, "targ"), (err, "err")):
        _want(t, torch.float32, n)
    batch, width = pred.shape
    assert tuple(targ.shape) == (batch, width) and err.numel() == batch, "pred, targ [B, E], err [B]"
    want = dpred is not None
    if want:
        _want(dpred, torch.float32, "dpred")
        _want(loss, torch.float32, "loss")
        assert dpred.numel() == batch * width and loss.numel() >= 1, "dpred [B, E], loss [1]"
    _check(load().arl_rnd_error(ptr(pred), ptr(targ), batch, width, int(want), ptr(err), ptr(dpred), ptr(loss),
                                stream_ptr(stream)), "arl_rnd_error")


def rnd_reward_mix(err, r_ext, n_env, horizon, rho, moments, gamma_int, c_ext, c_int, r_mix, diag2, workspace,
                   stream=None):
    """rho, the running moments of the discounted bonus and r_mix = c_ext r_ext + c_int err / std, in one launch."""
    for t, n in ((err, "err"), (r_ext, "r_ext"), (r_mix, "r_mix"), (diag2, "diag2")):
        _want(t, torch.float32, n)
    for t, n in ((rho, "rho"), (moments, "moments"), (workspace, "workspace")):
        _want(t, torch.float64, n)
    rows = n_env * horizon
    assert err.numel() == r_ext.numel() == r_mix.numel() == rows and rho.numel() == n_env and moments.numel() == 3 and \
        diag2.numel() >= 2 and workspace.numel() >= rows, "reward_mix sizes"
    _check(load().arl_rnd_reward_mix(ptr(err), ptr(r_ext), n_env, horizon, ptr(rho), ptr(moments), float(gamma_int),
                                     float(c_ext), float(c_int), ptr(r_mix), ptr(diag2), ptr(workspace),
                                     stream_ptr(stream)), "arl_rnd_reward_mix")


# ---------------------------------------------------------------------------
# PopArt: denormalised values for the scans, the statistics / head / target step (csrc/popart.hip)
# ---------------------------------------------------------------------------

def popart_denorm(value_n, last_n, stats, value, last_value, stream=None):
    """value = sigma * value_n + mu and last_value likewise from last_n, under stats f64[4] = (mu, nu, sigma, n_updates)."""
    for t, n in ((value_n, "value_n"), (last_n, "last_n"), (value, "value"), (last_value, "last_value")):
        _want(t, torch.float32, n)
    _want(stats, torch.float64, "stats")
    rows, n_last = value_n.numel(), last_n.numel()
    assert value.numel() == rows and last_value.numel() == n_last and stats.numel() == 4, "popart_denorm sizes"
    _check(load().arl_popart_denorm(ptr(value_n), rows, ptr(last_n), n_last, ptr(stats), ptr(value), ptr(last_value),
                                    stream_ptr(stream)), "arl_popart_denorm")


def popart_step(returns, advantages, valids, beta, sigma_min, sigma_max, stats, w_value, b_value, diag2, stream=None):
    """One launch: the batch's moments -> stats -> the value row / bias rewritten (outputs preserved) -> returns (and
    advantages, unless None) normalised in place; diag2 = (mu', sigma')."""
    for t, n in ((returns, "returns"), (w_value, "w_value"), (b_value, "b_value"), (diag2, "diag2")):
        _want(t, torch.float32, n)
    _want(stats, torch.float64, "stats")
    rows = returns.numel()
    if advantages is not None:
        _want(advantages, torch.float32, "advantages")
    if valids is not None:
        _want(valids, torch.int8, "valids")
    assert (advantages is None or advantages.numel() == rows) and (valids is None or valids.numel() == rows) and \
        stats.numel() == 4 and b_value.numel() == 1 and diag2.numel() >= 2, "popart_step sizes"
    _check(load().arl_popart_step(ptr(returns), ptr(advantages), ptr(valids), rows, float(beta), float(sigma_min),
                                  float(sigma_max), ptr(stats), ptr(w_value), ptr(b_value), w_value.numel(), ptr(diag2),
                                  stream_ptr(stream)), "arl_popart_step")


# ---------------------------------------------------------------------------
# R2D2: stored-state sequences on the replay memory and the sequence loss (csrc/r2d2.hip)
# ---------------------------------------------------------------------------

def _state_ptrs(tensors, name):
    for t in tensors:
        _want(t, torch.float32, name)
    return (C.c_void_p * max(len(tensors), 1))(*[ptr(t) for t in tensors])


def seq_store(state_in, resets, n_env, horizon, size, seq_stride, idx, state_store, reset_ring, stream=None):
    """One launch (arl_seq_store): the states recorded before every step of the batch whose ring index is a multiple of
    seq_stride -> state_store[s] f32[n_env, size / seq_stride, H]; every step's reset flag -> reset_ring u8[n_env, size].
    state_in: 0 .. 2 f32 [n_env * horizon, H] tensors (env-major); resets u8 / bool [n_env * horizon]; idx: the ring
    index of the batch's step 0."""
    if len(state_in) != len(state_store):
        raise ValueError("seq_store: %d states in, %d stores" % (len(state_in), len(state_store)))
    if resets.dtype == torch.bool:
        resets = resets.view(torch.uint8)
    _want(resets, torch.uint8, "resets")
    _want(reset_ring, torch.uint8, "reset_ring")
    hidden = state_in[0].shape[-1] if state_in else 0
    slots = size // max(seq_stride, 1)
    for a, b in zip(state_in, state_store):
        if a.numel() != n_env * horizon * hidden or b.numel() != n_env * slots * hidden:
            raise ValueError("seq_store: state shapes %s -> %s" % (tuple(a.shape), tuple(b.shape)))
    if resets.numel() != n_env * horizon or reset_ring.numel() != n_env * size:
        raise ValueError("seq_store: resets holds %d, the ring %d flags" % (resets.numel(), reset_ring.numel()))
    _check(load().arl_seq_store(_state_ptrs(state_in, "state_in"), len(state_in), hidden, ptr(resets), n_env, horizon,
                                size, seq_stride, idx, _state_ptrs(state_store, "state_store"), ptr(reset_ring),
                                stream_ptr(stream)), "arl_seq_store")


def seq_prepare(env, slot, seq_len, size, seq_stride, state_store, reset_ring, env_rows, step_rows, state_out, resets_out,
                stream=None):
    """One launch (arl_seq_prepare): (env, slot) i32[B] -> env_rows, step_rows i32[B * seq_len] (arl_replay_extract's
    lists), state_out[s] f32[B, H] <- state_store[s][env, slot], resets_out u8[B * seq_len] <- the ring's flags.  The
    caller guarantees env < n_env and slot < size / seq_stride."""
    for t, n in ((env, "env"), (slot, "slot"), (env_rows, "env_rows"), (step_rows, "step_rows")):
        _want(t, torch.int32, n)
    _want(reset_ring, torch.uint8, "reset_ring")
    _want(resets_out, torch.uint8, "resets_out")
    batch = env.numel()
    if len(state_out) != len(state_store):
        raise ValueError("seq_prepare: %d stores, %d states out" % (len(state_store), len(state_out)))
    if slot.numel() != batch or not env_rows.numel() == step_rows.numel() == resets_out.numel() == batch * seq_len:
        raise ValueError("seq_prepare: %d sequences of %d rows, lists of %d / %d / %d" % (
            batch, seq_len, env_rows.numel(), step_rows.numel(), resets_out.numel()))
    hidden = state_store[0].shape[-1] if state_store else 0
    for a, b in zip(state_store, state_out):
        if b.numel() != batch * hidden or a.numel() % max(hidden * (size // max(seq_stride, 1)), 1):
            raise ValueError("seq_prepare: state shapes %s -> %s" % (tuple(a.shape), tuple(b.shape)))
    _check(load().arl_seq_prepare(ptr(env), ptr(slot), batch, seq_len, size, seq_stride,
                                  _state_ptrs(state_store, "state_store"), len(state_store), hidden, ptr(reset_ring),
                                  ptr(env_rows), ptr(step_rows), _state_ptrs(state_out, "state_out"), ptr(resets_out),
                                  stream_ptr(stream)), "arl_seq_prepare")


def r2d2_loss(q, q_tgt, actions, returns, terminals, is_weights, batch, burn_in, train_len, n, n_actions, gamma_n,
              rescale_eps, eta, dq, td_abs, loss_rows, priorities, dueling=False, stream=None):
    """R2D2's loss, gradient and sequence priorities (arl_r2d2_loss): q, q_tgt, dq f32 [batch * U, q_stride] with
    U = burn_in + train_len + n, rows [sequence][time]; rescale_eps None or <= 0: no value rescaling."""
    for t, name in ((q, "q"), (q_tgt, "q_tgt"), (returns, "returns"), (dq, "dq"), (td_abs, "td_abs"),
                    (loss_rows, "loss_rows"), (priorities, "priorities")):
        _want(t, torch.float32, name)
    _want(actions, torch.uint8, "actions")
    _want_flags(terminals, "terminals")
    rows = batch * (burn_in + train_len + n)
    assert actions.numel() == returns.numel() == terminals.numel() == rows, "per-row input sizes"
    assert q.numel() == q_tgt.numel() == dq.numel() and q.numel() % rows == 0, "q / q_tgt / dq size"
    assert td_abs.numel() == batch * train_len and loss_rows.numel() == priorities.numel() == batch, "output sizes"
    if is_weights is not None:
        _want(is_weights, torch.float32, "is_weights")
        assert is_weights.numel() == batch, "is_weights size"
    _check(load().arl_r2d2_loss(ptr(q), ptr(q_tgt), ptr(actions), ptr(returns), ptr(terminals), ptr(is_weights), batch,
                                burn_in, train_len, n, n_actions, q.numel() // rows, int(dueling), float(gamma_n),
                                0.0 if rescale_eps is None else float(rescale_eps), float(eta), ptr(dq), ptr(td_abs),
                                ptr(loss_rows), ptr(priorities), stream_ptr(stream)), "arl_r2d2_loss")


# ---------------------------------------------------------------------------
# LayerNorm + rectifier (csrc/layernorm.hip)
# ---------------------------------------------------------------------------

def _ln_rows(z, gamma, same, stats):
    """(rows, width) of a LayerNorm call on z [rows][width] (any leading shape), after the size checks."""
    width = gamma.numel()
    rows = z.numel() // width
    assert rows * width == z.numel() and all(t.numel() == z.numel() for t in same), "activation sizes"
    assert stats.numel() == 2 * rows, "stats size"
    for t in (z, gamma, stats) + tuple(same):
        _want(t, torch.float32, "LayerNorm tensors")
    return rows, width


def ln_bwd_workspace(device):
    return torch.empty(load().arl_ln_bwd_workspace_bytes() // 4, dtype=torch.float32, device=device)


def ln_relu_fwd(z, gamma, beta, eps, y, stats, stream=None):
    """y = max(0, gamma * xhat(z) + beta) row-wise over z [.., width]; stats [rows, 2] = (mean, rstd); z is kept."""
    rows, width = _ln_rows(z, gamma, (y,), stats)
    assert beta.numel() == width, "beta size"
    _check(load().arl_ln_relu_fwd(ptr(z), ptr(gamma), ptr(beta), rows, width, float(eps), ptr(y), ptr(stats),
                                  stream_ptr(stream)), "arl_ln_relu_fwd")


def ln_relu_bwd(dy, y, z, stats, gamma, dy_masked, dz, dgamma, dbeta, workspace, stream=None):
    """dz (may be dy), dgamma, dbeta of ln_relu_fwd; the column sums are folded at once (FoldList.ln_relu_bwd defers)."""
    rows, width = _ln_rows(z, gamma, (dy, y, dz), stats)
    assert dgamma.numel() == dbeta.numel() == width, "dgamma / dbeta size"
    _check(load().arl_ln_relu_bwd(ptr(dy), ptr(y), ptr(z), ptr(stats), ptr(gamma), rows, width, int(bool(dy_masked)),
                                  ptr(dz), ptr(dgamma), ptr(dbeta), ptr(workspace), None, stream_ptr(stream)),
           "arl_ln_relu_bwd")


# ---------------------------------------------------------------------------
# Max pooling and the residual sum of the IMPALA residual network (csrc/resnet.hip); activations NHWC
# ---------------------------------------------------------------------------

def maxpool3s2_out_hw(in_h, in_w):
    return (in_h - 1) // 2 + 1, (in_w - 1) // 2 + 1


def _pool_dims(z, y):
    """(batch, in_h, in_w, channels) of a pooling call on z [B, H, W, C] and y [B, Ho, Wo, C], after the shape checks."""
    b, h, w, c = z.shape
    assert tuple(y.shape) == (b,) + maxpool3s2_out_hw(h, w) + (c,), "pooled shape"
    return b, h, w, c


def maxpool3s2_fwd(z, y, y_relu=None, arg=None, stream=None):
    """y = the 3 x 3 / stride 2 / pad 1 maximum of z f32[B, H, W, C]; y_relu = max(y, 0); arg u8 = the window position
    3 ky + kx of the first maximum (maxpool3s2_bwd's input)."""
    b, h, w, c = _pool_dims(z, y)
    _want(z, torch.float32, "z")
    _want(y, torch.float32, "y")
    if y_relu is not None:
        _want(y_relu, torch.float32, "y_relu")
        assert y_relu.shape == y.shape, "y_relu shape"
    if arg is not None:
        _want(arg, torch.uint8, "arg")
        assert arg.shape == y.shape, "arg shape"
    _check(load().arl_maxpool3s2_fwd(ptr(z), b, h, w, c, ptr(y), ptr(y_relu), ptr(arg), stream_ptr(stream)),
           "arl_maxpool3s2_fwd")


def maxpool3s2_bwd(dy, arg, dz, stream=None):
    """dz f32[B, H, W, C] = the gradient of maxpool3s2_fwd's input, given dy and arg of its output's shape."""
    b, h, w, c = _pool_dims(dz, dy)
    _want(dy, torch.float32, "dy")
    _want(dz, torch.float32, "dz")
    _want(arg, torch.uint8, "arg")
    assert arg.shape == dy.shape, "arg shape"
    _check(load().arl_maxpool3s2_bwd(ptr(dy), ptr(arg), b, h, w, c, ptr(dz), stream_ptr(stream)), "arl_maxpool3s2_bwd")


def gather_scale_obs_nhwc_any(obs, idx, out, scale, stream=None):
    """obs u8[n,C,H,W] (rows optionally picked by idx) -> out f32 with NHWC memory, [B,H,W,C rounded up to 4] contiguous,
    the padding channels zero; any C, H, W (gather_scale_obs_nhwc: the fast path of four 16-byte-multiple planes)."""
    _want(obs, torch.uint8, "obs")
    _want(out, torch.float32, "out")
    if idx is not None:
        _want(idx, torch.int32, "idx")
        assert idx.numel() == out.shape[0], "idx length"
    else:
        assert obs.shape[0] == out.shape[0], "obs rows"
    batch = out.shape[0]
    channels, plane = obs.shape[1], obs.shape[2] * obs.shape[3]
    assert out.numel() == batch * plane * ((channels + 3) // 4 * 4), "out size"
    _check(load().arl_gather_scale_obs_nhwc_any(ptr(obs), ptr(idx), batch, channels, plane, float(scale), out.data_ptr(),
                                                stream_ptr(stream)), "arl_gather_scale_obs_nhwc_any")


def add_relu(a, b, out, relu=None, stream=None):
    """out = a + b (out may be a or b); relu = max(out, 0) when given."""
    for t in (a, b, out) + (() if relu is None else (relu,)):
        _want(t, torch.float32, "add_relu tensors")
        assert t.numel() == a.numel(), "sizes"
    _check(load().arl_add_relu(ptr(a), ptr(b), a.numel(), ptr(out), ptr(relu), stream_ptr(stream)), "arl_add_relu")


# ---------------------------------------------------------------------------
# LSTM cell (csrc/lstm.hip).  Tensors may be row-strided views ([B, cols] with stride(1) == 1).
# ---------------------------------------------------------------------------

def _rows(t):
    """(data_ptr, row stride in elements) of a 2-D tensor whose rows are contiguous."""
    if t is None:
        return None, 0
    assert t.dim() == 2 and t.stride(1) == 1 and t.is_cuda and t.dtype == torch.float32
    return t.data_ptr(), t.stride(0)


def lstm_cell_fwd(gx, gh, c_prev, h_out, c_out, gates=None, stream=None):
    batch, hidden = c_prev.shape
    (pgx, sgx), (pcp, scp), (ph, sh), (pc, sc), (pg, sg) = _rows(gx), _rows(c_prev), _rows(h_out), _rows(c_out), _rows(gates)
    _check(load().arl_lstm_cell_fwd(pgx, sgx, ptr(gh), pcp, scp, batch, hidden, ph, sh, pc, sc, pg, sg,
                                    stream_ptr(stream)), "arl_lstm_cell_fwd")


def lstm_cell_bwd(dh, dh_rec, dc_next, gates, c_prev, c_out, dgates, dc_prev, stream=None):
    batch, hidden = c_prev.shape
    (pdh, sdh), (pg, sg), (pcp, scp), (pc, sc), (pdg, sdg) = _rows(dh), _rows(gates), _rows(c_prev), _rows(c_out), _rows(dgates)
    _check(load().arl_lstm_cell_bwd(pdh, sdh, ptr(dh_rec), ptr(dc_next), pg, sg, pcp, scp, pc, sc, batch, hidden,
                                    pdg, sdg, ptr(dc_prev), stream_ptr(stream)), "arl_lstm_cell_bwd")


def gru_cell_fwd(gx, gh, h_prev, h_out, saved=None, stream=None):
    batch, hidden = h_prev.shape
    (pgx, sgx), (php, shp), (ph, sh), (ps, ss) = _rows(gx), _rows(h_prev), _rows(h_out), _rows(saved)
    _check(load().arl_gru_cell_fwd(pgx, sgx, ptr(gh), php, shp, batch, hidden, ph, sh, ps, ss, stream_ptr(stream)),
           "arl_gru_cell_fwd")


def gru_cell_bwd(dh, dh_rec, dh_dir, saved, h_prev, dgx, dgh, dh_prev, stream=None):
    batch, hidden = h_prev.shape
    (pdh, sdh), (ps, ss), (php, shp), (pgx, sgx), (pgh, sgh) = _rows(dh), _rows(saved), _rows(h_prev), _rows(dgx), _rows(dgh)
    _check(load().arl_gru_cell_bwd(pdh, sdh, ptr(dh_rec), ptr(dh_dir), ps, ss, php, shp, batch, hidden, pgx, sgx,
                                   pgh, sgh, ptr(dh_prev), stream_ptr(stream)), "arl_gru_cell_bwd")


def rnn_cell_fwd(gx, gh, h_out, stream=None):
    batch, hidden = h_out.shape
    (pgx, sgx), (ph, sh) = _rows(gx), _rows(h_out)
    _check(load().arl_rnn_cell_fwd(pgx, sgx, ptr(gh), batch, hidden, ph, sh, stream_ptr(stream)), "arl_rnn_cell_fwd")


def rnn_cell_bwd(dh, dh_rec, h_out, dpre, stream=None):
    batch, hidden = h_out.shape
    (pdh, sdh), (ph, sh), (pd, sd) = _rows(dh), _rows(h_out), _rows(dpre)
    _check(load().arl_rnn_cell_bwd(pdh, sdh, ptr(dh_rec), ph, sh, batch, hidden, pd, sd, stream_ptr(stream)),
           "arl_rnn_cell_bwd")


# ---------------------------------------------------------------------------
# reset-aware BPTT (csrc/handover.hip and the *_cell_bwd_reset entry points of csrc/lstm.hip, csrc/gru.hip).
# flags = (reset u8[rows of the full batch], idx i32 row map or None, row0, row_step): launch row b reads the flag of
# compact row row0 + b * row_step (include/accel_rl_hip.h).
# ---------------------------------------------------------------------------

def _flags(flags, batch):
    reset, idx, row0, row_step = flags
    if reset.dtype == torch.bool:
        reset = reset.view(torch.uint8)
    _want(reset, torch.uint8, "reset")
    last = row0 + (batch - 1) * row_step
    if idx is not None:
        _want(idx, torch.int32, "idx")
        if not 0 <= row0 <= last < idx.numel():
            raise ValueError("flag rows %d .. %d outside the row map's %d rows" % (row0, last, idx.numel()))
    elif not 0 <= row0 <= last < reset.numel():
        raise ValueError("flag rows %d .. %d outside the %d flags" % (row0, last, reset.numel()))
    return ptr(reset), ptr(idx), row0, row_step


def seq_handover(h_prev, c_prev, flags, hp, hprev_out, cprev_out=None, stream=None):
    """hp, hprev_out <- h_prev and cprev_out <- c_prev where the row's flag is clear, zero where it is set
    (arl_seq_handover: the state of step t-1 handed to step t; flags address the rows of step t-1)."""
    batch, hidden = h_prev.shape
    (ph, sh), (pc, sc), (po, so), (pco, sco) = _rows(h_prev), _rows(c_prev), _rows(hprev_out), _rows(cprev_out)
    assert tuple(hp.shape) == (batch, hidden) and hp.dtype == torch.float32
    pr, pi, row0, step = _flags(flags, batch)
    _check(load().arl_seq_handover(ph, sh, pc, sc, pr, pi, row0, step, batch, hidden, ptr(hp), po, so, pco, sco,
                                   stream_ptr(stream)), "arl_seq_handover")


def lstm_cell_bwd_reset(dh, dh_rec, dc_next, gates, c_prev, c_out, dgates, dc_prev, flags, stream=None):
    batch, hidden = c_prev.shape
    (pdh, sdh), (pg, sg), (pcp, scp), (pc, sc), (pdg, sdg) = _rows(dh), _rows(gates), _rows(c_prev), _rows(c_out), _rows(dgates)
    pr, pi, row0, step = _flags(flags, batch)
    _check(load().arl_lstm_cell_bwd_reset(pdh, sdh, ptr(dh_rec), ptr(dc_next), pg, sg, pcp, scp, pc, sc, batch, hidden,
                                          pdg, sdg, ptr(dc_prev), pr, pi, row0, step, stream_ptr(stream)),
           "arl_lstm_cell_bwd_reset")


def gru_cell_bwd_reset(dh, dh_rec, dh_dir, saved, h_prev, dgx, dgh, dh_prev, flags, stream=None):
    batch, hidden = h_prev.shape
    (pdh, sdh), (ps, ss), (php, shp), (pgx, sgx), (pgh, sgh) = _rows(dh), _rows(saved), _rows(h_prev), _rows(dgx), _rows(dgh)
    pr, pi, row0, step = _flags(flags, batch)
    _check(load().arl_gru_cell_bwd_reset(pdh, sdh, ptr(dh_rec), ptr(dh_dir), ps, ss, php, shp, batch, hidden, pgx, sgx,
                                         pgh, sgh, ptr(dh_prev), pr, pi, row0, step, stream_ptr(stream)),
           "arl_gru_cell_bwd_reset")


def rnn_cell_bwd_reset(dh, dh_rec, h_out, dpre, flags, stream=None):
    batch, hidden = h_out.shape
    (pdh, sdh), (ph, sh), (pd, sd) = _rows(dh), _rows(h_out), _rows(dpre)
    pr, pi, row0, step = _flags(flags, batch)
    _check(load().arl_rnn_cell_bwd_reset(pdh, sdh, ptr(dh_rec), ph, sh, batch, hidden, pd, sd, pr, pi, row0, step,
                                         stream_ptr(stream)), "arl_rnn_cell_bwd_reset")


# ---------------------------------------------------------------------------
# noisy dense layers (csrc/noisy.hip)
# ---------------------------------------------------------------------------

def noisy_normals(seed, counter, layer, which, rows, width, rows_per_draw=1, e=None, f=None, words=None, stream=None):
    """One noisy layer's e_in (which 0) or e_out (which 1) draw, exactly as a forward pass makes it (arl_noisy_normals):
    e, f = f(e) f32[rows][width], words int32[rows][width] (the Philox word each element used, as raw bits)."""
    for t, dt, n in ((e, torch.float32, "e"), (f, torch.float32, "f"), (words, torch.int32, "words")):
        if t is not None:
            _want(t, dt, n)
            assert t.numel() == rows * width, "%s size" % n
    _check(load().arl_noisy_normals(int(seed), int(counter), int(layer), int(which), int(rows), int(width),
                                    int(rows_per_draw), ptr(e), ptr(f), ptr(words), stream_ptr(stream)),
           "arl_noisy_normals")


def noisy_noise(state, layers, rows, rows_per_draw, stream=None):
    """layers: [(fein, feout, x or None, xs or None, fan_in, units, out_stride, layer)] -> one arl_noisy_noise launch."""
    _want(state, torch.int64, "state")
    assert 0 < len(layers) <= NOISY_MAX_LAYERS
    arr = (ArlNoisyLayer * len(layers))()
    for it, (fein, feout, x, xs, fan_in, units, out_stride, layer) in zip(arr, layers):
        assert fein.numel() == rows * fan_in and feout.numel() == rows * out_stride, "noise buffer sizes"
        assert x is None or (x.numel() == xs.numel() == rows * fan_in), "x / xs size"
        it.fein, it.feout, it.x, it.xs = ptr(fein), ptr(feout), ptr(x), ptr(xs)
        it.fan_in, it.units, it.out_stride, it.layer = fan_in, units, out_stride, layer
    _check(load().arl_noisy_noise(ptr(state), arr, len(layers), rows, rows_per_draw, stream_ptr(stream)),
           "arl_noisy_noise")


def noisy_dense_combine(w_item, bias, s_item, b_sigma, feout, y, relu, fein_next=None, xs_next=None, state=None,
                        stream=None):
    """y[rows, units] = relu?(P_w + f(e_out) * P_sigma) from the two conv2d_fwd_parts items (arl_noisy_dense_combine)."""
    rows, units = y.shape
    assert feout.numel() == y.numel(), "feout size"
    assert fein_next is None or (fein_next.numel() == xs_next.numel() == y.numel()), "fein_next / xs_next size"
    _check(load().arl_noisy_dense_combine(C.byref(w_item), ptr(bias), C.byref(s_item), ptr(b_sigma), ptr(feout), rows,
                                          units, int(bool(relu)), ptr(y), ptr(fein_next), ptr(xs_next), ptr(state),
                                          stream_ptr(stream)), "arl_noisy_dense_combine")


def noisy_dense_bwd_prep(g, feout, g2, db, db_sigma, stream=None):
    rows, units = g.shape
    assert feout.numel() == g2.numel() == g.numel() and db.numel() == db_sigma.numel() == units, "sizes"
    _check(load().arl_noisy_dense_bwd_prep(ptr(g), ptr(feout), rows, units, ptr(g2), ptr(db), ptr(db_sigma),
                                           stream_ptr(stream)), "arl_noisy_dense_bwd_prep")


def noisy_dense_bwd_dx(dx_w, dx_sigma, fein, dx, stream=None):
    rows, fan_in = dx.shape[0], dx.numel() // dx.shape[0]
    assert dx_w.numel() == dx_sigma.numel() == fein.numel() == dx.numel(), "sizes"
    _check(load().arl_noisy_dense_bwd_dx(ptr(dx_w), ptr(dx_sigma), ptr(fein), rows, fan_in, ptr(dx),
                                         stream_ptr(stream)), "arl_noisy_dense_bwd_dx")


def noisy_draws(state, draws, rows, rows_per_draw, stream=None):
    """draws: [(f, x or None, xs or None, width, pitch, layer, which)] -> one arl_noisy_draws launch.  f / x / xs may be
    column slices of wider buffers (pitch floats per row)."""
    _want(state, torch.int64, "state")
    assert 0 < len(draws) <= NOISY_MAX_DRAWS
    arr = (ArlNoisyDraw * len(draws))()
    for it, (f, x, xs, width, pitch, layer, which) in zip(arr, draws):
        for t in (f, x, xs):                # (column slices: not contiguous, rows `pitch` floats apart)
            assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == rows and
                                 t.shape[1] >= width and t.stride() == (pitch, 1)), "draw buffer shape / pitch"
        it.f, it.x, it.xs = (None if t is None else t.data_ptr() for t in (f, x, xs))
        it.width, it.pitch, it.layer, it.which = width, pitch, layer, which
    _check(load().arl_noisy_draws(ptr(state), arr, len(draws), rows, rows_per_draw, stream_ptr(stream)),
           "arl_noisy_draws")


def noisy_duel_combine(w_item, bias, s_lo, s_hi, b_sigma, feout, y, split, relu, fein_next=None, xs_next=None,
                       state=None, stream=None):
    """y[rows, units] = relu?(P_w + f(e_out) * P_sigma), P_sigma from s_lo (columns < split) / s_hi (the rest)."""
    rows, units = y.shape
    assert feout.numel() == y.numel(), "feout size"
    assert fein_next is None or (fein_next.numel() == xs_next.numel() == y.numel()), "fein_next / xs_next size"
    _check(load().arl_noisy_duel_combine(C.byref(w_item), ptr(bias), C.byref(s_lo), C.byref(s_hi), ptr(b_sigma),
                                         ptr(feout), rows, units, split, int(bool(relu)), ptr(y), ptr(fein_next),
                                         ptr(xs_next), ptr(state), stream_ptr(stream)), "arl_noisy_duel_combine")


def noisy_duel_bwd_prep(g, feout, split, g2_lo, g2_hi, db, db_sigma, stream=None):
    rows, units = g.shape
    assert feout.numel() == g.numel() and db.numel() == db_sigma.numel() == units, "sizes"
    assert g2_lo.numel() == rows * split and g2_hi.numel() == rows * (units - split), "g2 sizes"
    _check(load().arl_noisy_duel_bwd_prep(ptr(g), ptr(feout), rows, units, split, ptr(g2_lo), ptr(g2_hi), ptr(db),
                                          ptr(db_sigma), stream_ptr(stream)), "arl_noisy_duel_bwd_prep")


def noisy_duel_bwd_dx(dx_w, dxs_lo, fein_lo, dxs_hi, fein_hi, dx, stream=None):
    rows, fan_in = dx.shape[0], dx.numel() // dx.shape[0]
    assert all(t.numel() == dx.numel() for t in (dx_w, dxs_lo, fein_lo, dxs_hi, fein_hi)), "sizes"
    _check(load().arl_noisy_duel_bwd_dx(ptr(dx_w), ptr(dxs_lo), ptr(fein_lo), ptr(dxs_hi), ptr(fein_hi), rows, fan_in,
                                        ptr(dx), stream_ptr(stream)), "arl_noisy_duel_bwd_dx")


def noisy_catdqn_loss_limits():
    """(max splits per product, max actions, max atoms) of arl_noisy_catdqn_loss_parts."""
    v = [C.c_int32() for _ in range(3)]
    _check(load().arl_noisy_catdqn_loss_limits(*(C.byref(x) for x in v)), "arl_noisy_catdqn_loss_limits")
    return tuple(x.value for x in v)


def noisy_logit_src(w_item, bias, s_item, b_sigma, feout, row0=0, row_floats=0):
    """ArlNoisyLogitSrc from the output layer's two conv2d_fwd_parts items, its biases and f(e_out), rows from row0 on."""
    src = ArlNoisyLogitSrc()
    off = 4 * row0 * row_floats
    src.w_part, src.s_part = w_item.part + off, s_item.part + off
    src.bias_or_null, src.b_sigma_or_null = ptr(bias), ptr(b_sigma)
    src.feout = feout.data_ptr() + off
    src.w_split_stride, src.s_split_stride = w_item.total, s_item.total
    src.w_splits, src.s_splits = w_item.splits, s_item.splits
    return src


def noisy_catdqn_loss_parts(pred, tgt_next, pol_next, z, actions, returns, terminals, is_weights, n_actions, n_atoms,
                            atom_stride, v_min, v_max, gamma_n, dlogits, loss_rows, kl, dueling=False, stream=None,
                            dgrad_weights=None):
    """arl_catdqn_loss on a noisy output layer's two products (ArlNoisyLogitSrc each; pol_next None: not double DQN)."""
    wt_items, n_wt = None, 0
    if dgrad_weights:
        n_wt = len(dgrad_weights)
        assert n_wt <= DGRAD_WT_MAX
        wt_items = (ArlDgradWt * n_wt)()
        for it, (w, wt, geom) in zip(wt_items, dgrad_weights):
            it.w, it.wt, it.geom = ptr(w), ptr(wt), C.pointer(geom)
    _check(load().arl_noisy_catdqn_loss_parts(C.byref(pred), C.byref(tgt_next),
                                              None if pol_next is None else C.byref(pol_next), ptr(z), ptr(actions),
                                              ptr(returns), ptr(terminals), ptr(is_weights), actions.numel(), n_actions,
                                              n_atoms, atom_stride, int(dueling), float(v_min), float(v_max),
                                              float(gamma_n), ptr(dlogits), ptr(loss_rows), ptr(kl), wt_items, n_wt,
                                              stream_ptr(stream)), "arl_noisy_catdqn_loss_parts")
