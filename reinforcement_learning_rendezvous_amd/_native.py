"""
ctypes binding of librdv_hip.so — the C ABI declared in include/rdv.h.

There is no CPU fallback: if the library is missing or no HIP device is usable, the calls raise.
"""
import ctypes as C
import os
import subprocess

from .params import EnvParams

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "librdv_hip.so")
CSRC = os.path.join(_PKG, "csrc")

STORAGE_F32, STORAGE_F64 = 0, 1
ON_DONE_RESET, ON_DONE_HALT, ON_DONE_CONTINUE = 0, 1, 2
VARIANT_AUTO, VARIANT_FUSED, VARIANT_SPLIT, VARIANT_FUSED_INLANE, VARIANT_FUSED_TILES = 0, 1, 2, 3, 4
OBS_DIM, ACT_DIM, STATE_DIM, DIAG_DIM, AUX_DIM, EVAL_DIM = 17, 6, 20, 8, 8, 32

ERROR_NAMES = {0: "RDV_OK", -1: "RDV_ERR_INVALID_ARGUMENT", -2: "RDV_ERR_NO_DEVICE", -3: "RDV_ERR_HIP",
               -4: "RDV_ERR_OUT_OF_MEMORY", -5: "RDV_ERR_BAD_HANDLE", -6: "RDV_ERR_BAD_PARAMS", -7: "RDV_ERR_DEVICE_FAULT"}
DEVERR_LOST_SIGNAL = 1

# every symbol include/rdv.h declares (tests/test_abi.py checks the list against the header and the .so)
SYMBOLS = ["rdv_version", "rdv_last_error", "rdv_device_error_code", "rdv_debug_set_device_error", "rdv_debug_last_kernel", "rdv_params_default", "rdv_params_validate", "rdv_workspace_bytes",
           "rdv_create", "rdv_destroy", "rdv_set_params", "rdv_get_params", "rdv_seed", "rdv_set_reset_tape",
           "rdv_set_kernel_variant", "rdv_rigid_body_default", "rdv_set_rigid_body", "rdv_get_rigid_body",
           "rdv_reset", "rdv_step", "rdv_step_many", "rdv_set_state", "rdv_get_state", "rdv_get_aux", "rdv_snapshot_bytes", "rdv_snapshot", "rdv_restore", "rdv_observe", "rdv_diagnose",
           "rdv_eval_begin", "rdv_eval_summary", "rdv_get_stats", "rdv_num_envs", "rdv_policy_create", "rdv_policy_destroy", "rdv_policy_act", "rdv_critic_create", "rdv_policy_value", "rdv_rollout",
           # parameter groups (added within ABI 5)
           "rdv_param_groups_check", "rdv_param_groups_validate", "rdv_set_param_groups", "rdv_set_group_params", "rdv_get_group_params",
           "rdv_num_groups", "rdv_get_group_stats", "rdv_eval_group_summary",
           # other MLP architectures (added within ABI 5)
           "rdv_mlp_spec_default", "rdv_mlp_spec_check", "rdv_policy_create_mlp", "rdv_critic_create_mlp", "rdv_policy_get_spec",
           # learner-ready rollouts (added within ABI 5)
           "rdv_gae", "rdv_rollout_advantages", "rdv_policy_set_weights",
           # policy sets (added within ABI 5)
           "rdv_policy_set_create", "rdv_critic_set_create", "rdv_policy_set_member_weights", "rdv_policy_num_members", "rdv_policy_num_rows",
           # the recurrent policy (added within ABI 5)
           "rdv_lstm_spec_check", "rdv_lstm_policy_create", "rdv_lstm_critic_create", "rdv_lstm_act", "rdv_lstm_value", "rdv_lstm_get_state",
           "rdv_lstm_set_state", "rdv_lstm_reset_state", "rdv_lstm_set_weights", "rdv_lstm_hidden_size",
           # recurrent policy sets (added within ABI 5)
           "rdv_lstm_policy_set_create", "rdv_lstm_critic_set_create", "rdv_lstm_set_member_weights",
           # PPO minibatch gradients (added within ABI 5)
           "rdv_ppo_workspace_bytes", "rdv_ppo_spec_check", "rdv_ppo_loss_grad",
           # PPO minibatch gradients for policy sets (added within ABI 5)
           "rdv_ppo_set_workspace_bytes", "rdv_ppo_set_loss_grad",
           # gradient clip, Adam and weight repack for policy sets (added within ABI 5)
           "rdv_ppo_set_adam_step", "rdv_policy_block_floats", "rdv_policy_get_block",
           # PPO minibatch gradients for every MLP architecture (added within ABI 5)
           "rdv_ppo_mlp_spec_check", "rdv_ppo_mlp_grad_floats", "rdv_ppo_mlp_workspace_bytes", "rdv_ppo_mlp_loss_grad",
           # PPO minibatch gradients for policy sets of every MLP architecture (added within ABI 5)
           "rdv_ppo_mlp_set_spec_check", "rdv_ppo_mlp_set_workspace_bytes", "rdv_ppo_mlp_set_loss_grad",
           # gradient clip, Adam and weight repack for policy sets of every MLP architecture (added within ABI 5)
           "rdv_ppo_mlp_set_adam_step",
           # recurrent PPO minibatch gradients (added within ABI 5)
           "rdv_lstm_ppo_spec_check", "rdv_lstm_ppo_grad_floats", "rdv_lstm_ppo_workspace_bytes", "rdv_lstm_ppo_loss_grad",
           # recurrent PPO minibatch gradients for recurrent sets (added within ABI 5)
           "rdv_lstm_ppo_set_workspace_bytes", "rdv_lstm_ppo_set_loss_grad",
           # gradient clip, Adam and weight repack for recurrent policy sets (added within ABI 5)
           "rdv_lstm_ppo_adam_workspace_bytes", "rdv_lstm_ppo_set_adam_step"]


class RdvError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


class StepOut(C.Structure):
    """RdvStepOut"""
    _fields_ = [("obs", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("terminal_obs", C.c_void_p),
                ("episode_return", C.c_void_p), ("episode_length", C.c_void_p), ("done_reason", C.c_void_p),
                ("diag", C.c_void_p), ("eval", C.c_void_p)]


class Stats(C.Structure):
    """RdvStats"""
    _fields_ = [("env_steps", C.c_uint64), ("episodes", C.c_uint64), ("successes", C.c_uint64),
                ("collisions", C.c_uint64), ("reasons", C.c_uint64 * 4), ("sum_return", C.c_double),
                ("sum_length", C.c_double), ("sum_delta_v", C.c_double), ("sum_delta_w", C.c_double)]

    def to_dict(self):
        return dict(env_steps=int(self.env_steps), episodes=int(self.episodes), successes=int(self.successes),
                    collisions=int(self.collisions), reasons=[int(x) for x in self.reasons],
                    sum_return=float(self.sum_return), sum_length=float(self.sum_length),
                    sum_delta_v=float(self.sum_delta_v), sum_delta_w=float(self.sum_delta_w))


class EvalSummary(C.Structure):
    """RdvEvalSummary: the twelve means custom_callbacks.evaluate_policy logs (:285-298)"""
    _fields_ = [(k, C.c_double) for k in ("ep_rew", "ep_len", "ep_dist", "ep_delta_v", "ep_delta_w", "ep_success", "ep_collision_percentage",
                                           "ep_time_of_first_collision", "ep_min_pos_error", "ep_avg_att_error", "pct_collided_episodes",
                                           "pct_successful_episodes")] + [("episodes", C.c_int64)]


class RolloutOut(C.Structure):
    """RdvRolloutOut: device pointers of the rollout-buffer rows"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("log_prob", C.c_void_p), ("last_obs", C.c_void_p)]


class AdvantageOut(C.Structure):
    """RdvAdvantageOut: device pointers of the rollout-buffer columns rdv_rollout_advantages writes"""
    _fields_ = [("values", C.c_void_p), ("last_value", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p)]


class PpoRows(C.Structure):
    """RdvPpoRows: flat device views of a rollout's rows, and the minibatch's row indices (nullable)"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("old_log_prob", C.c_void_p), ("advantages", C.c_void_p),
                ("returns", C.c_void_p), ("indices", C.c_void_p), ("rows", C.c_int64)]


class PpoOut(C.Structure):
    """RdvPpoOut: device pointers of what rdv_ppo_loss_grad / rdv_ppo_mlp_loss_grad write (log_prob and values nullable)"""
    _fields_ = [("actor_grad", C.c_void_p), ("critic_grad", C.c_void_p), ("scalars", C.c_void_p), ("log_prob", C.c_void_p),
                ("values", C.c_void_p)]


class LstmPpoRows(C.Structure):
    """RdvLstmPpoRows: device pointers of a recurrent rollout's [T,N,...] columns, the two state0 pairs [N,H] and the minibatch's env
    columns (nullable)"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("old_log_prob", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
                ("done", C.c_void_p), ("actor_h0", C.c_void_p), ("actor_c0", C.c_void_p), ("critic_h0", C.c_void_p), ("critic_c0", C.c_void_p),
                ("envs", C.c_void_p), ("n_envs", C.c_int64), ("n_steps", C.c_int64), ("n_seq", C.c_int64)]


class LstmPpoOut(C.Structure):
    """RdvLstmPpoOut: device pointers of what rdv_lstm_ppo_loss_grad writes (log_prob and values [T, n_seq] nullable)"""
    _fields_ = [("actor_grad", C.c_void_p), ("critic_grad", C.c_void_p), ("scalars", C.c_void_p), ("log_prob", C.c_void_p),
                ("values", C.c_void_p)]


class LstmPpoSetOut(C.Structure):
    """RdvLstmPpoSetOut: device pointers of what rdv_lstm_ppo_set_loss_grad writes: [P,Ga], [P,Gc], [P,8]; log_prob and values: member g's
    [T, B_g] block at float T off_g, nullable"""
    _fields_ = [("actor_grad", C.c_void_p), ("critic_grad", C.c_void_p), ("scalars", C.c_void_p), ("log_prob", C.c_void_p),
                ("values", C.c_void_p)]


class PpoSetOut(C.Structure):
    """RdvPpoSetOut: device pointers of what rdv_ppo_set_loss_grad writes: [P,5708], [P,5377], [P,8]; log_prob and values [sum of counts], nullable"""
    _fields_ = [("actor_grad", C.c_void_p), ("critic_grad", C.c_void_p), ("scalars", C.c_void_p), ("log_prob", C.c_void_p),
                ("values", C.c_void_p)]


class AdamState(C.Structure):
    """RdvAdamState: device pointers of the fp32 master weights [P,5708] / [P,5377], the Adam moments, the step counters [P] (int64) and
    the coefficient rows [P,8] that rdv_ppo_set_adam_step writes"""
    _fields_ = [("actor_param", C.c_void_p), ("critic_param", C.c_void_p), ("actor_m", C.c_void_p), ("actor_v", C.c_void_p),
                ("critic_m", C.c_void_p), ("critic_v", C.c_void_p), ("step", C.c_void_p), ("coef", C.c_void_p)]


PPO_ACTOR_GRAD, PPO_CRITIC_GRAD, PPO_SCALARS = 5708, 5377, 8
POLICY_BLOCK_FLOATS, POLICY_BLOCK_STD = 8372, 8352     # kPolFloats, kPolStd (csrc/rdv_policy.h): the shipped block and its six exp(log_std) floats
ADAM_COEF = 8
ADAM_COEF_NAMES = ("total_norm", "clip_coef", "step_size", "inv_sqrt_bc2", "skipped")
PPO_SCALAR_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")

ACT_TANH, ACT_RELU, ACT_SIGMOID = 0, 1, 2
MLP_MAX_HIDDEN = 4


class MlpSpec(C.Structure):
    """RdvMlpSpec: 1..4 hidden layers of 16, 32 or 64, one RdvActivation for the whole network"""
    _fields_ = [("n_hidden", C.c_int32), ("hidden", C.c_int32 * MLP_MAX_HIDDEN), ("activation", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, hidden, activation=ACT_TANH):
        """(rdv_mlp_spec_check judges it: more than MLP_MAX_HIDDEN widths are cut to the array and keep their count)"""
        hidden = [int(x) for x in hidden]
        return cls(len(hidden), (C.c_int32 * MLP_MAX_HIDDEN)(*hidden[:MLP_MAX_HIDDEN]), int(activation), 0)

    def to_tuple(self):
        return self.n_hidden, list(self.hidden), self.activation


class LstmSpec(C.Structure):
    """RdvLstmSpec: one LSTM layer of 32 / 64 / 128 / 256 units in front of an RdvMlpSpec trunk, separate actor and critic LSTMs"""
    _fields_ = [("hidden_size", C.c_int32), ("n_layers", C.c_int32), ("shared", C.c_int32), ("reserved", C.c_int32), ("trunk", MlpSpec)]

    @classmethod
    def make(cls, hidden_size, trunk, activation=ACT_TANH, n_layers=1, shared=0):
        return cls(int(hidden_size), int(n_layers), int(shared), 0, MlpSpec.make(trunk, activation))


INTEGRATORS = {"auto": 0, "exact": 1, "rk45": 2}


class RigidBody(C.Structure):
    """RdvRigidBody: self.inertia / self.inertia_target (rendezvous_env.py:75-79, :96-100; row-major 3x3), the body torques
    of integrate_*_attitude (:552, :579) and the tolerances of the env's solve_ivp calls (:567-568)."""
    _fields_ = [("inertia_chaser", C.c_double * 9), ("inertia_target", C.c_double * 9), ("torque_chaser", C.c_double * 3),
                ("torque_target", C.c_double * 3), ("rtol", C.c_double), ("atol", C.c_double),
                ("integrator", C.c_int32), ("reserved", C.c_int32)]


def build(force=False, quiet=True):
    """Compile the fourteen translation units of csrc/ (rdv_hip.hip, rdv_tiles.hip, rdv_general.hip, rdv_groups.hip, rdv_policy_mlp.hip, rdv_policy_lstm.hip, rdv_policy_sets.hip, rdv_advantages.hip, rdv_ppo.hip, rdv_ppo_mlp.hip, rdv_ppo_lstm.hip, rdv_ppo_adam.hip, rdv_ppo_lstm_adam.hip and the host-only rdv_policy_host.hip) for gfx950 and link librdv_hip.so
    (hipcc cross-compiles without a GPU).  `make` owns the dependency list (every header of csrc/ and include/rdv.h): it is always
    asked, and rebuilds only what is out of date."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL if quiet else None)
    return LIB_PATH


_lib = None
STRICT = True      # tools/lib_ab*.py load OLDER builds of the library for A/B timings and switch this off; the product never does


def lib():
    """Load librdv_hip.so and declare the signatures of include/rdv.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RdvError(-2, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the product has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i64, u64, i32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32
    PP = C.POINTER(EnvParams)
    sig = {
        "rdv_version": (C.c_int, []),
        "rdv_last_error": (C.c_char_p, []),
        "rdv_device_error_code": (C.c_int, [C.c_uint32]),
        "rdv_debug_set_device_error": (C.c_int, [vp, C.c_uint32, vp]),
        "rdv_debug_last_kernel": (C.c_char_p, [vp]),
        "rdv_params_default": (C.c_int, [PP]),
        "rdv_params_validate": (C.c_int, [PP]),
        "rdv_workspace_bytes": (i64, [i64, C.c_int]),
        "rdv_create": (C.c_int, [PP, i64, C.c_int, C.c_int, C.c_int, u64, u64, vp, C.POINTER(vp)]),
        "rdv_destroy": (C.c_int, [vp]),
        "rdv_set_params": (C.c_int, [vp, PP, vp]),
        "rdv_get_params": (C.c_int, [vp, PP]),
        "rdv_seed": (C.c_int, [vp, u64]),
        "rdv_set_reset_tape": (C.c_int, [vp, vp, i32]),
        "rdv_set_kernel_variant": (C.c_int, [vp, C.c_int]),
        "rdv_rigid_body_default": (C.c_int, [C.POINTER(RigidBody)]),
        "rdv_set_rigid_body": (C.c_int, [vp, C.POINTER(RigidBody), vp]),
        "rdv_get_rigid_body": (C.c_int, [vp, C.POINTER(RigidBody)]),
        "rdv_reset": (C.c_int, [vp, vp, vp, vp]),
        "rdv_step": (C.c_int, [vp, vp, C.POINTER(StepOut), vp]),
        "rdv_step_many": (C.c_int, [vp, vp, i32, C.POINTER(StepOut), vp]),
        "rdv_set_state": (C.c_int, [vp, vp, vp]),
        "rdv_get_state": (C.c_int, [vp, vp, vp]),
        "rdv_get_aux": (C.c_int, [vp, vp, vp]),
        "rdv_snapshot_bytes": (i64, [vp]),
        "rdv_snapshot": (C.c_int, [vp, vp, vp]),
        "rdv_restore": (C.c_int, [vp, vp, i64, vp]),
        "rdv_observe": (C.c_int, [vp, vp, vp]),
        "rdv_diagnose": (C.c_int, [vp, vp, vp]),
        "rdv_eval_begin": (C.c_int, [vp, vp, vp]),
        "rdv_eval_summary": (C.c_int, [vp, vp, C.POINTER(EvalSummary), vp]),
        "rdv_get_stats": (C.c_int, [vp, C.POINTER(Stats), C.c_int, vp]),
        "rdv_num_envs": (i64, [vp]),
        "rdv_policy_create": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_policy_destroy": (C.c_int, [vp]),
        "rdv_policy_act": (C.c_int, [vp, vp, vp, i64, C.c_int, u64, u64, u64, vp]),
        "rdv_critic_create": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_policy_value": (C.c_int, [vp, vp, vp, i64, vp]),
        "rdv_rollout": (C.c_int, [vp, vp, i32, C.POINTER(RolloutOut), C.c_int, u64, u64, vp]),
        "rdv_param_groups_check": (C.c_int, [i64, i32, C.POINTER(i64)]),
        "rdv_param_groups_validate": (C.c_int, [PP, i32]),
        "rdv_set_param_groups": (C.c_int, [vp, PP, C.POINTER(i64), i32, vp]),
        "rdv_set_group_params": (C.c_int, [vp, i32, PP, vp]),
        "rdv_get_group_params": (C.c_int, [vp, i32, PP]),
        "rdv_num_groups": (i32, [vp]),
        "rdv_get_group_stats": (C.c_int, [vp, C.POINTER(Stats), C.c_int, vp]),
        "rdv_eval_group_summary": (C.c_int, [vp, i32, vp, C.POINTER(EvalSummary), vp]),
        "rdv_mlp_spec_default": (C.c_int, [C.POINTER(MlpSpec)]),
        "rdv_mlp_spec_check": (C.c_int, [C.POINTER(MlpSpec)]),
        "rdv_policy_create_mlp": (C.c_int, [C.POINTER(MlpSpec), vp, vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_critic_create_mlp": (C.c_int, [C.POINTER(MlpSpec), vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_policy_get_spec": (C.c_int, [vp, C.POINTER(MlpSpec)]),
        "rdv_gae": (C.c_int, [vp, vp, vp, vp, i32, i64, C.c_double, C.c_double, vp, vp, C.c_int, vp]),
        "rdv_rollout_advantages": (C.c_int, [vp, C.POINTER(RolloutOut), i32, i64, C.c_double, C.c_double, C.POINTER(AdvantageOut), vp]),
        "rdv_policy_set_weights": (C.c_int, [vp, vp, vp, vp, vp]),
        "rdv_policy_set_create": (C.c_int, [C.POINTER(MlpSpec), i32, C.POINTER(i64), vp, vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_critic_set_create": (C.c_int, [C.POINTER(MlpSpec), i32, C.POINTER(i64), vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_policy_set_member_weights": (C.c_int, [vp, i32, vp, vp, vp, vp]),
        "rdv_policy_num_members": (i32, [vp]),
        "rdv_policy_num_rows": (i64, [vp]),
        "rdv_lstm_spec_check": (C.c_int, [C.POINTER(LstmSpec)]),
        "rdv_lstm_policy_create": (C.c_int, [C.POINTER(LstmSpec), vp, vp, vp, vp, vp, vp, vp, i64, C.c_int, C.POINTER(vp)]),
        "rdv_lstm_critic_create": (C.c_int, [C.POINTER(LstmSpec), vp, vp, vp, vp, vp, vp, i64, C.c_int, C.POINTER(vp)]),
        "rdv_lstm_act": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, C.c_int, u64, u64, u64, vp]),
        "rdv_lstm_value": (C.c_int, [vp, vp, vp, vp, i64, C.c_int, vp]),
        "rdv_lstm_get_state": (C.c_int, [vp, vp, vp, vp]),
        "rdv_lstm_set_state": (C.c_int, [vp, vp, vp, vp]),
        "rdv_lstm_reset_state": (C.c_int, [vp, vp, vp]),
        "rdv_lstm_set_weights": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rdv_lstm_hidden_size": (i32, [vp]),
        "rdv_lstm_policy_set_create": (C.c_int, [C.POINTER(LstmSpec), i32, C.POINTER(i64), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_lstm_critic_set_create": (C.c_int, [C.POINTER(LstmSpec), i32, C.POINTER(i64), vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]),
        "rdv_lstm_set_member_weights": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rdv_ppo_workspace_bytes": (i64, [i64]),
        "rdv_ppo_spec_check": (C.c_int, [C.POINTER(MlpSpec), C.POINTER(MlpSpec)]),
        "rdv_ppo_loss_grad": (C.c_int, [vp, vp, C.POINTER(PpoRows), i64, C.c_double, C.c_double, C.c_double, vp, i64, C.POINTER(PpoOut), vp]),
        "rdv_ppo_set_workspace_bytes": (i64, [i32, C.POINTER(i64)]),
        "rdv_ppo_set_loss_grad": (C.c_int, [vp, vp, C.POINTER(PpoRows), C.POINTER(i64), C.c_double, C.c_double, C.c_double, vp, i64, C.POINTER(PpoSetOut), vp]),
        "rdv_ppo_set_adam_step": (C.c_int, [vp, vp, C.POINTER(AdamState), vp, vp, u64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
        "rdv_policy_block_floats": (i64, [vp]),
        "rdv_policy_get_block": (C.c_int, [vp, i32, vp, i64, vp]),
        "rdv_ppo_mlp_spec_check": (C.c_int, [C.POINTER(MlpSpec), C.POINTER(MlpSpec)]),
        "rdv_ppo_mlp_grad_floats": (i64, [C.POINTER(MlpSpec), C.c_int]),
        "rdv_ppo_mlp_workspace_bytes": (i64, [C.POINTER(MlpSpec), C.POINTER(MlpSpec), i64]),
        "rdv_ppo_mlp_loss_grad": (C.c_int, [vp, vp, C.POINTER(PpoRows), i64, C.c_double, C.c_double, C.c_double, vp, i64, C.POINTER(PpoOut), vp]),
        "rdv_ppo_mlp_set_spec_check": (C.c_int, [C.POINTER(MlpSpec), C.POINTER(MlpSpec)]),
        "rdv_ppo_mlp_set_workspace_bytes": (i64, [C.POINTER(MlpSpec), C.POINTER(MlpSpec), i32, C.POINTER(i64)]),
        "rdv_ppo_mlp_set_loss_grad": (C.c_int, [vp, vp, C.POINTER(PpoRows), C.POINTER(i64), C.c_double, C.c_double, C.c_double, vp, i64, C.POINTER(PpoSetOut), vp]),
        "rdv_ppo_mlp_set_adam_step": (C.c_int, [vp, vp, C.POINTER(AdamState), vp, vp, u64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
        "rdv_lstm_ppo_spec_check": (C.c_int, [C.POINTER(LstmSpec), C.POINTER(LstmSpec)]),
        "rdv_lstm_ppo_grad_floats": (i64, [C.POINTER(LstmSpec), C.c_int]),
        "rdv_lstm_ppo_workspace_bytes": (i64, [C.POINTER(LstmSpec), C.POINTER(LstmSpec), i64, i64]),
        "rdv_lstm_ppo_loss_grad": (C.c_int, [vp, vp, C.POINTER(LstmPpoRows), C.c_double, C.c_double, C.c_double, vp, i64, C.POINTER(LstmPpoOut), vp]),
        "rdv_lstm_ppo_set_workspace_bytes": (i64, [C.POINTER(LstmSpec), C.POINTER(LstmSpec), i64, C.c_int32, C.POINTER(i64)]),
        "rdv_lstm_ppo_set_loss_grad": (C.c_int, [vp, vp, C.POINTER(LstmPpoRows), C.POINTER(i64), C.c_double, C.c_double, C.c_double, vp, i64,
                                                 C.POINTER(LstmPpoSetOut), vp]),
        "rdv_lstm_ppo_adam_workspace_bytes": (i64, [C.POINTER(LstmSpec), C.POINTER(LstmSpec), C.c_int32]),
        "rdv_lstm_ppo_set_adam_step": (C.c_int, [vp, vp, C.POINTER(AdamState), vp, vp, u64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                                 vp, i64, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name, None)
        if fn is None:
            if STRICT:
                raise RdvError(-2, f"{LIB_PATH} does not export {name}: it is not a build of this source tree (ABI 5)")
            continue
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(code):
    if code != 0:
        raise RdvError(code, lib().rdv_last_error().decode("utf-8", "replace"))
    return code
