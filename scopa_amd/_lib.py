"""ctypes binding of libscopa_hip.so (the C ABI declared in include/scopa.h).

The product path: every solver entry point goes through this library's HIP kernels.  There is no
Python or CPU fallback -- if the library is missing or no GPU is present the call raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCOPA_HIP_LIBRARY: another build of the same sources (the host-only AddressSanitizer/UBSan build of `make -C tests/tools asan`);
# never a fallback -- a path that does not exist fails exactly like the default one
LIB_PATH = os.environ.get("SCOPA_HIP_LIBRARY") or os.path.join(_HERE, "libscopa_hip.so")

SCOPA_OK, SCOPA_EINVAL, SCOPA_ENODEV, SCOPA_EHIP, SCOPA_ESTATE, SCOPA_ENOMEM, SCOPA_ELIMIT, SCOPA_ETIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7
N_NODES, N_DECISION, N_TERMINAL = 2229, 1653, 576
TEAM_N_CHOICE, TEAM_N_LEAVES, TEAM_N_INFOSETS = 321365, 331776, 1648469   # include/scopa.h: SCOPA_TEAM_N_*
TEAM_SDCFR_ROWS, TEAM_SDCFR_VISITS = 1653, (4277, 3127)   # include/scopa.h: SCOPA_TEAM_SDCFR_*: memory rows / non-terminal visits of one Deep CFR traversal (per traverser)
TEAM_MCCFR_DRAWS = (49381, 20583)   # decision visits (np.random.choice draws) of one reference traversal per traverser; 69 964 per iteration()

# every symbol include/scopa.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "scopa_abi_version", "scopa_strerror", "scopa_last_error", "scopa_ctx_create", "scopa_ctx_destroy",
    "scopa_ctx_synchronize", "scopa_deal_py_seed", "scopa_state_init", "scopa_state_step", "scopa_state_clone", "scopa_state_is_terminal",
    "scopa_state_current_player", "scopa_state_legal", "scopa_state_rewards_x2", "scopa_state_infoset_key",
    "scopa_key_to_string", "scopa_state_infoset_string", "scopa_step_batch", "scopa_step_batch_host", "scopa_set_deal",
    "scopa_tree_counts", "scopa_tree_export", "scopa_tables_reset", "scopa_tables_get", "scopa_tables_set",
    "scopa_visited_get", "scopa_cfr_exact_iterate", "scopa_cfr_exact_traverse", "scopa_cfr_exact_mode", "scopa_cfr_exact_last_route", "scopa_cfr_exact_traverse_from", "scopa_mccfr_replay", "scopa_mccfr_seed",
    "scopa_mccfr_iterate", "scopa_mccfr_traverse", "scopa_mccfr_delta_buffer", "scopa_mccfr_bind_delta", "scopa_mccfr_delta_get", "scopa_mccfr_delta_set", "scopa_mccfr_apply",
    "scopa_mccfr_iteration_counter", "scopa_mccfr_graph_mode", "scopa_debug_lds_limit", "scopa_sdcfr_frontier_width", "scopa_sdcfr_features", "scopa_sdcfr_expand",
    "scopa_sdcfr_terminal_values", "scopa_sdcfr_backward", "scopa_sdcfr_visits", "scopa_sdcfr_policy_get", "scopa_sdcfr_traverse_fused", "scopa_sdcfr_image_floats", "scopa_sdcfr_pack_weights", "scopa_sdcfr_tuning", "scopa_sdcfr_mode", "scopa_sdcfr_train_params", "scopa_sdcfr_train_step", "scopa_sdcfr_train_steps", "scopa_sdcfr_average_policy", "scopa_features_from_states",
    "scopa_eval_init_states", "scopa_eval_step", "scopa_eval_tabular_step", "scopa_eval_tabular_prepare", "scopa_eval_tabular_match", "scopa_cfr_sync_iterate", "scopa_cfr_sync_iterate_weighted", "scopa_multi_create", "scopa_multi_destroy",
    "scopa_multi_deal_py_seeds", "scopa_multi_set_perms", "scopa_multi_perms_get", "scopa_multi_build", "scopa_multi_cfr_exact_iterate",
    "scopa_multi_cfr_exact_iterate_lanes", "scopa_multi_cfr_sync_iterate", "scopa_multi_cfr_sync_iterate_weighted", "scopa_multi_mccfr_iterate", "scopa_multi_exploitability", "scopa_multi_tables_get", "scopa_multi_tables_set", "scopa_multi_counters",
    "scopa_chance_create", "scopa_chance_destroy", "scopa_chance_counts", "scopa_chance_index_get", "scopa_chance_tables_reset", "scopa_chance_tables_get", "scopa_chance_tables_set",
    "scopa_chance_cfr_iterate_weighted", "scopa_chance_cfr_iterate_sampled", "scopa_chance_mccfr_iterate", "scopa_chance_mccfr_counters", "scopa_chance_exploitability", "scopa_chance_policy_for_deal",
    "scopa_chance_cross_play", "scopa_chance_best_response", "scopa_chance_debug_scratch_budget", "scopa_chance_match",
    "scopa_chance_sdcfr_traverse", "scopa_chance_sdcfr_visits", "scopa_chance_sdcfr_average_policy", "scopa_full_deal_py_seed",
    "scopa_full_state_init", "scopa_full_state_step", "scopa_full_state_legal", "scopa_full_state_infoset_string",
    "scopa_full_step_batch", "scopa_full_step_batch_host", "scopa_full_random_playouts",
    "scopa_full_infoset_key", "scopa_full_mccfr_create", "scopa_full_mccfr_destroy", "scopa_full_mccfr_root", "scopa_full_mccfr_cut", "scopa_full_mccfr_reset",
    "scopa_full_mccfr_traverse", "scopa_full_mccfr_apply", "scopa_full_mccfr_iterate", "scopa_full_mccfr_counters", "scopa_full_mccfr_tables_get",
    "scopa_full_mccfr_delta_get", "scopa_full_mccfr_tables_set", "scopa_full_mccfr_match", "scopa_full_mccfr_exploitability", "scopa_full_mccfr_response_get",
    "scopa_full_infoset_key_wide", "scopa_full_chance_create", "scopa_full_chance_destroy", "scopa_full_chance_root", "scopa_full_chance_cut", "scopa_full_chance_reset",
    "scopa_full_chance_traverse", "scopa_full_chance_apply", "scopa_full_chance_iterate", "scopa_full_chance_counters", "scopa_full_chance_tables_get",
    "scopa_full_chance_delta_get", "scopa_full_chance_tables_set", "scopa_full_chance_match", "scopa_full_chance_exploitability", "scopa_full_chance_response_get", "scopa_full_chance_cfr_iterate",
    "scopa_full_chance_cross_play", "scopa_full_chance_pair_match",
    "scopa_full_chance_respond_traverse", "scopa_full_chance_respond_iterate", "scopa_full_chance_harden",
    "scopa_full_chance_respond_nets_traverse", "scopa_full_chance_respond_nets_iterate",
    "scopa_full_chance_sdcfr_features", "scopa_full_chance_sdcfr_traverse", "scopa_full_chance_sdcfr_visits", "scopa_full_chance_sdcfr_policy_get", "scopa_full_chance_sdcfr_average_policy", "scopa_full_chance_debug_sdcfr",
    "scopa_full_chance_sdcfr_traverse_frontier", "scopa_full_chance_sdcfr_policy_at", "scopa_full_chance_debug_sdcfr_scratch", "scopa_full_chance_sdcfr_average_at", "scopa_full_chance_sdcfr_match", "scopa_full_chance_debug_sdcfr_average_grid",
    "scopa_full_sdcfr_train_params", "scopa_full_sdcfr_train_steps",
    "scopa_team_state_init", "scopa_team_state_step", "scopa_team_state_legal", "scopa_team_state_rewards_x2", "scopa_team_state_infoset_string",
    "scopa_team_step_batch", "scopa_team_step_batch_host", "scopa_team_random_playouts",
    "scopa_team_set_deal", "scopa_team_tree_counts", "scopa_team_tree_leaves", "scopa_team_tables_reset", "scopa_team_tables_get", "scopa_team_tables_set",
    "scopa_team_cfr_iterate", "scopa_team_cfr_traverse", "scopa_team_cfr_launch", "scopa_team_exploitability", "scopa_team_minimax", "scopa_team_policy_value",
    "scopa_team_chance_create", "scopa_team_chance_destroy", "scopa_team_chance_debug_image_budget", "scopa_team_chance_counts", "scopa_team_chance_index_get",
    "scopa_team_chance_tables_reset", "scopa_team_chance_tables_get", "scopa_team_chance_tables_set", "scopa_team_chance_sigma_get", "scopa_team_chance_cfr_iterate", "scopa_team_chance_cfr_iterate_sampled", "scopa_team_chance_cfr_launch",
    "scopa_team_chance_exploitability", "scopa_team_chance_policy_for_deal",
    "scopa_team_chance_mccfr_traverse", "scopa_team_chance_mccfr_apply", "scopa_team_chance_mccfr_walk", "scopa_team_chance_mccfr_iterate", "scopa_team_chance_mccfr_counters", "scopa_team_chance_mccfr_delta_get",
    "scopa_team_cross_play", "scopa_team_match", "scopa_team_debug_xplay_group_limit", "scopa_team_chance_cross_play", "scopa_team_chance_match",
    "scopa_team_chance_sdcfr_traverse", "scopa_team_chance_sdcfr_visits", "scopa_team_chance_sdcfr_policy_get", "scopa_team_chance_sdcfr_forced_get", "scopa_team_chance_sdcfr_average_policy", "scopa_team_chance_debug_sdcfr",
    "scopa_team_mccfr_replay", "scopa_team_mccfr_traverse", "scopa_team_mccfr_apply", "scopa_team_mccfr_iterate", "scopa_team_mccfr_counters", "scopa_team_mccfr_delta_get", "scopa_team_mccfr_visits_get",
    "scopa_mccfr_iterate_sharded", "scopa_p2p_create", "scopa_p2p_connect", "scopa_p2p_allreduce_delta", "scopa_p2p_set_form", "scopa_p2p_set_budget", "scopa_p2p_status", "scopa_p2p_destroy", "scopa_exploitability", "scopa_cross_play", "scopa_best_response", "scopa_eval_pair_match", "scopa_counters", "scopa_prof_enable", "scopa_prof_read", "scopa_prof_device", "scopa_prof_phases", "scopa_prof_spread",
]


class ScopaError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        msg = f"{where}: status {status}"
        try:
            msg += f" ({lib().scopa_strerror(status).decode()})"
        except Exception:
            pass
        if detail:
            msg += f": {detail}"
        super().__init__(msg)


class State16(C.Structure):
    """scopa_state, 16 bytes (include/scopa.h)."""
    _fields_ = [("hand", C.c_uint16 * 2), ("table", C.c_uint32), ("nh", C.c_uint8 * 2), ("nt", C.c_uint8),
                ("step", C.c_uint8), ("ncap", C.c_uint8 * 2), ("scopas", C.c_uint8 * 2)]


STEP_CLONED, STEP_COUNT_MASK = 0x80, 0x7F   # include/scopa.h: SCOPA_STEP_CLONED, SCOPA_STEP_COUNT_MASK
STATE_DTYPE = np.dtype([("hand", "<u2", (2,)), ("table", "<u4"), ("nh", "u1", (2,)), ("nt", "u1"), ("step", "u1"),
                        ("ncap", "u1", (2,)), ("scopas", "u1", (2,))])
assert STATE_DTYPE.itemsize == 16 and C.sizeof(State16) == 16

_lib = None


def lib():
    """Load the library (raises OSError loudly if it has not been built: python -m scopa_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # PyTorch-ROCm bundles its own HIP/HSA runtime.  If libscopa_hip.so pulled in /opt/rocm's copy first, torch would
        # later start a SECOND runtime in the process and find no GPU; loading torch first makes both share one.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` or `python scopa_amd/build.py` "
                      "(the MiniScopa solver path has no fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
    sig = {
        "scopa_abi_version": (i32, []),
        "scopa_strerror": (C.c_char_p, [i32]),
        "scopa_last_error": (C.c_char_p, [vp]),
        "scopa_ctx_create": (i32, [i32, vp, C.POINTER(vp)]),
        "scopa_ctx_destroy": (i32, [vp]),
        "scopa_ctx_synchronize": (i32, [vp]),
        "scopa_deal_py_seed": (i32, [i64, vp]),
        "scopa_state_init": (i32, [vp, C.POINTER(State16)]),
        "scopa_state_step": (i32, [C.POINTER(State16), i32]),
        "scopa_state_clone": (i32, [C.POINTER(State16), C.POINTER(State16)]),
        "scopa_state_is_terminal": (i32, [C.POINTER(State16)]),
        "scopa_state_current_player": (i32, [C.POINTER(State16)]),
        "scopa_state_legal": (i32, [C.POINTER(State16), i32, C.POINTER(i32 * 4), C.POINTER(i32)]),
        "scopa_state_rewards_x2": (i32, [C.POINTER(State16), C.POINTER(i32 * 2)]),
        "scopa_state_infoset_key": (i32, [C.POINTER(State16), i32, C.POINTER(u64)]),
        "scopa_key_to_string": (i32, [u64, C.c_char_p, i32]),
        "scopa_state_infoset_string": (i32, [C.POINTER(State16), i32, C.c_char_p, i32]),
        "scopa_step_batch": (i32, [vp, vp, vp, i64]),
        "scopa_step_batch_host": (i32, [vp, vp, vp, i64]),
        "scopa_set_deal": (i32, [vp, vp]),
        "scopa_tree_counts": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "scopa_tree_export": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "scopa_tables_reset": (i32, [vp]),
        "scopa_tables_get": (i32, [vp, vp, vp, vp]),
        "scopa_tables_set": (i32, [vp, vp, vp, vp]),
        "scopa_cfr_exact_iterate": (i32, [vp, i32, vp]),
        "scopa_cfr_exact_traverse": (i32, [vp, i32, C.POINTER(C.c_double)]),
        "scopa_cfr_exact_mode": (i32, [vp, i32]),
        "scopa_cfr_exact_last_route": (i32, [vp, C.POINTER(i32)]),
        "scopa_cfr_exact_traverse_from": (i32, [vp, i32, i32, vp, C.c_double, C.c_double, C.POINTER(C.c_double)]),
        "scopa_visited_get": (i32, [vp, vp]),
        "scopa_mccfr_replay": (i32, [vp, i32, vp, i64, C.POINTER(i64)]),
        "scopa_mccfr_seed": (i32, [vp, u64]),
        "scopa_mccfr_iterate": (i32, [vp, u32, u32]),
        "scopa_mccfr_traverse": (i32, [vp, u32, u32, u32]),
        "scopa_mccfr_delta_buffer": (i32, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "scopa_mccfr_bind_delta": (i32, [vp, vp, C.c_size_t]),
        "scopa_mccfr_delta_get": (i32, [vp, vp]),
        "scopa_mccfr_delta_set": (i32, [vp, vp]),
        "scopa_mccfr_apply": (i32, [vp]),
        "scopa_mccfr_iteration_counter": (i32, [vp, C.POINTER(u32)]),
        "scopa_mccfr_graph_mode": (i32, [vp, i32]),
        "scopa_debug_lds_limit": (i32, [vp, i32]),
        "scopa_exploitability": (i32, [vp, vp, vp, vp]),
        "scopa_sdcfr_frontier_width": (i32, [i32, i32]),
        "scopa_sdcfr_features": (i32, [vp, i32, i64, vp, vp, vp]),
        "scopa_sdcfr_expand": (i32, [vp, i32, i32, i64, vp, vp, vp, vp, vp, u32, u32]),
        "scopa_sdcfr_terminal_values": (i32, [vp, i32, i64, vp, vp]),
        "scopa_sdcfr_backward": (i32, [vp, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64]),
        "scopa_sdcfr_visits": (i32, [vp, C.POINTER(u64)]),
        "scopa_sdcfr_policy_get": (i32, [vp, vp, vp]),
        "scopa_sdcfr_traverse_fused": (i32, [vp, i32, i32, vp, vp, vp, vp, i64, i64, vp, vp, u32, u32]),
        "scopa_sdcfr_image_floats": (i32, []),
        "scopa_sdcfr_pack_weights": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "scopa_sdcfr_tuning": (i32, [vp, i32, i32]),
        "scopa_sdcfr_train_params": (i32, []),
        "scopa_sdcfr_train_step": (i32, [vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, C.c_float, vp]),
        "scopa_sdcfr_train_steps": (i32, [vp, vp, i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, C.c_float, vp]),
        "scopa_full_sdcfr_train_params": (i32, []),
        "scopa_full_sdcfr_train_steps": (i32, [vp, vp, i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, C.c_float, vp]),
        "scopa_sdcfr_mode": (i32, [vp, i32]),
        "scopa_sdcfr_average_policy": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
        "scopa_features_from_states": (i32, [vp, vp, i64, vp, vp]),
        "scopa_eval_init_states": (i32, [vp, vp, i64]),
        "scopa_eval_step": (i32, [vp, vp, i64, vp, vp, u32, u32]),
        "scopa_eval_tabular_step": (i32, [vp, vp, vp, i64, i32, vp, vp, u32]),
        "scopa_eval_tabular_prepare": (i32, [vp, vp]),
        "scopa_eval_tabular_match": (i32, [vp, i64, i64, u32, vp, vp, vp]),
        "scopa_cross_play": (i32, [vp, i32, vp, vp]),
        "scopa_best_response": (i32, [vp, i32, vp, vp, vp]),
        "scopa_eval_pair_match": (i32, [vp, vp, vp, i64, i64, u32, vp, vp]),
        "scopa_cfr_sync_iterate": (i32, [vp, i32]),
        "scopa_cfr_sync_iterate_weighted": (i32, [vp, i32, vp, i32]),
        "scopa_multi_create": (i32, [vp, i32, C.POINTER(vp)]),
        "scopa_multi_destroy": (i32, [vp]),
        "scopa_multi_deal_py_seeds": (i32, [vp, vp]),
        "scopa_multi_set_perms": (i32, [vp, vp]),
        "scopa_multi_perms_get": (i32, [vp, vp]),
        "scopa_multi_build": (i32, [vp, vp]),
        "scopa_multi_cfr_exact_iterate": (i32, [vp, i32]),
        "scopa_multi_cfr_sync_iterate": (i32, [vp, i32]),
        "scopa_multi_cfr_sync_iterate_weighted": (i32, [vp, i32, vp, i32, vp]),
        "scopa_multi_cfr_exact_iterate_lanes": (i32, [vp, i32]),
        "scopa_multi_exploitability": (i32, [vp, vp]),
        "scopa_multi_mccfr_iterate": (i32, [vp, u32, u32, u64]),
        "scopa_multi_tables_get": (i32, [vp, i32, vp, vp, vp, vp]),
        "scopa_multi_tables_set": (i32, [vp, i32, vp, vp, vp]),
        "scopa_multi_counters": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "scopa_chance_create": (i32, [vp, C.POINTER(vp)]),
        "scopa_chance_destroy": (i32, [vp]),
        "scopa_chance_counts": (i32, [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]),
        "scopa_chance_index_get": (i32, [vp, vp, vp]),
        "scopa_chance_tables_reset": (i32, [vp]),
        "scopa_chance_tables_get": (i32, [vp, vp, vp]),
        "scopa_chance_tables_set": (i32, [vp, vp, vp]),
        "scopa_chance_cfr_iterate_weighted": (i32, [vp, i32, vp, i32]),
        "scopa_chance_cfr_iterate_sampled": (i32, [vp, i32, i32, vp, vp, i32]),
        "scopa_chance_mccfr_iterate": (i32, [vp, i32, u32, u64, i32, vp]),
        "scopa_chance_mccfr_counters": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]),
        "scopa_chance_exploitability": (i32, [vp, vp, vp, vp]),
        "scopa_chance_policy_for_deal": (i32, [vp, vp, i32, vp]),
        "scopa_chance_cross_play": (i32, [vp, i32, vp, vp, vp]),
        "scopa_chance_best_response": (i32, [vp, i32, vp, vp, vp]),
        "scopa_chance_debug_scratch_budget": (i32, [vp, i64]),
        "scopa_chance_match": (i32, [vp, vp, vp, i64, i64, u32, vp, vp, vp]),
        "scopa_chance_sdcfr_traverse": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, i64, vp, u32, u32]),
        "scopa_chance_sdcfr_visits": (i32, [vp, C.POINTER(u64)]),
        "scopa_chance_sdcfr_average_policy": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
        "scopa_full_deal_py_seed": (i32, [i64, vp]),
        "scopa_full_state_init": (i32, [vp, u32, vp]),
        "scopa_full_state_step": (i32, [vp, vp, i32]),
        "scopa_full_state_legal": (i32, [vp, i32, C.POINTER(i32 * 3), C.POINTER(i32)]),
        "scopa_full_state_infoset_string": (i32, [vp, i32, C.c_char_p, i32]),
        "scopa_full_step_batch": (i32, [vp, vp, vp, vp, i64]),
        "scopa_full_step_batch_host": (i32, [vp, vp, vp, vp, i64, i64]),
        "scopa_full_random_playouts": (i32, [vp, vp, i64, vp, vp]),
        "scopa_full_infoset_key": (i32, [vp, vp, i32, C.POINTER(u64)]),
        "scopa_full_mccfr_create": (i32, [vp, vp, vp, i32, C.POINTER(vp)]),
        "scopa_full_mccfr_destroy": (i32, [vp]),
        "scopa_full_mccfr_root": (i32, [vp, vp, vp, C.POINTER(i32)]),
        "scopa_full_mccfr_cut": (i32, [vp, i32]),
        "scopa_full_mccfr_reset": (i32, [vp]),
        "scopa_full_mccfr_traverse": (i32, [vp, i32, u32, u32, u32]),
        "scopa_full_mccfr_apply": (i32, [vp]),
        "scopa_full_mccfr_iterate": (i32, [vp, u32, u32]),
        "scopa_full_mccfr_counters": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]),
        "scopa_full_mccfr_tables_get": (i32, [vp, C.POINTER(i64), vp, vp, vp, vp]),
        "scopa_full_mccfr_delta_get": (i32, [vp, C.POINTER(i64), vp, vp, vp, vp]),
        "scopa_full_mccfr_tables_set": (i32, [vp, i64, vp, vp, vp, vp]),
        "scopa_full_mccfr_match": (i32, [vp, i64, u32, vp, vp]),
        "scopa_full_mccfr_exploitability": (i32, [vp, vp, i32, vp]),
        "scopa_full_mccfr_response_get": (i32, [vp, i32, C.POINTER(i64), vp, vp, vp, vp]),
        "scopa_full_infoset_key_wide": (i32, [vp, i32, C.POINTER(u64 * 2)]),
        "scopa_full_chance_create": (i32, [vp, vp, i32, vp, i32, C.POINTER(vp)]),
        "scopa_full_chance_destroy": (i32, [vp]),
        "scopa_full_chance_root": (i32, [vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]),
        "scopa_full_chance_cut": (i32, [vp, i32]),
        "scopa_full_chance_reset": (i32, [vp]),
        "scopa_full_chance_traverse": (i32, [vp, i32, u32, u32, u32, vp, i32]),
        "scopa_full_chance_apply": (i32, [vp]),
        "scopa_full_chance_iterate": (i32, [vp, u32, u32, vp, i32]),
        "scopa_full_chance_counters": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]),
        "scopa_full_chance_tables_get": (i32, [vp, C.POINTER(i64), vp, vp, vp, vp]),
        "scopa_full_chance_delta_get": (i32, [vp, C.POINTER(i64), vp, vp, vp, vp]),
        "scopa_full_chance_tables_set": (i32, [vp, i64, vp, vp, vp, vp]),
        "scopa_full_chance_match": (i32, [vp, i64, u32, vp, i32, vp, vp]),
        "scopa_full_chance_exploitability": (i32, [vp, vp, vp, i32, i32, vp]),
        "scopa_full_chance_response_get": (i32, [vp, i32, C.POINTER(i64), vp, vp, vp, vp]),
        "scopa_full_chance_cfr_iterate": (i32, [vp, vp, i32, vp, i32, vp]),
        "scopa_full_chance_sdcfr_features": (i32, [vp, i64, vp]),
        "scopa_full_chance_sdcfr_traverse": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, u32, u32]),
        "scopa_full_chance_sdcfr_traverse_frontier": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, u32, u32]),
        "scopa_full_chance_sdcfr_policy_at": (i32, [vp, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "scopa_full_chance_debug_sdcfr_scratch": (i32, [vp, i64]),
        "scopa_full_chance_sdcfr_average_at": (i32, [vp, i32, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "scopa_full_chance_debug_sdcfr_average_grid": (i32, [vp, i32]),
        "scopa_full_chance_sdcfr_match": (i32, [vp, i64, u32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "scopa_full_chance_sdcfr_visits": (i32, [vp, C.POINTER(u64)]),
        "scopa_full_chance_debug_sdcfr": (i32, [vp, i32]),
        "scopa_full_chance_sdcfr_policy_get": (i32, [vp, C.POINTER(i64), vp, vp, vp]),
        "scopa_full_chance_sdcfr_average_policy": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(i64), vp, vp]),
        "scopa_full_chance_cross_play": (i32, [vp, i32, vp, vp, i32, i32, vp]),
        "scopa_full_chance_pair_match": (i32, [vp, vp, i64, u32, vp, i32, vp, vp]),
        "scopa_full_chance_respond_traverse": (i32, [vp, vp, i32, i32, u32, u32, u32, vp, i32]),
        "scopa_full_chance_respond_iterate": (i32, [vp, vp, i32, u32, u32, vp, i32]),
        "scopa_full_chance_harden": (i32, [vp]),
        "scopa_full_chance_respond_nets_traverse": (i32, [vp, vp, i32, u32, vp, i32, vp, u32, u32]),
        "scopa_full_chance_respond_nets_iterate": (i32, [vp, vp, u32, u32, vp, i32]),
        "scopa_mccfr_iterate_sharded": (i32, [vp, u32, u32, u32]),
        "scopa_p2p_create": (i32, [vp, i32, i32, vp]),
        "scopa_p2p_connect": (i32, [vp, vp]),
        "scopa_p2p_allreduce_delta": (i32, [vp]),
        "scopa_p2p_set_form": (i32, [vp, i32]),
        "scopa_p2p_set_budget": (i32, [vp, C.c_double]),
        "scopa_p2p_status": (i32, [vp, C.POINTER(i32), C.POINTER(u64)]),
        "scopa_p2p_destroy": (i32, [vp]),
        "scopa_team_state_init": (i32, [vp, vp]),
        "scopa_team_state_step": (i32, [vp, i32]),
        "scopa_team_state_legal": (i32, [vp, C.POINTER(i32 * 4), C.POINTER(i32)]),
        "scopa_team_state_rewards_x2": (i32, [vp, C.POINTER(i32 * 4)]),
        "scopa_team_state_infoset_string": (i32, [vp, i32, C.c_char_p, i32]),
        "scopa_team_step_batch": (i32, [vp, vp, vp, i64]),
        "scopa_team_step_batch_host": (i32, [vp, vp, vp, i64]),
        "scopa_team_random_playouts": (i32, [vp, vp, i64, vp, vp]),
        "scopa_team_set_deal": (i32, [vp, vp]),
        "scopa_team_tree_counts": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "scopa_team_tree_leaves": (i32, [vp, vp]),
        "scopa_team_tables_reset": (i32, [vp]),
        "scopa_team_tables_get": (i32, [vp, vp, vp, vp, vp]),
        "scopa_team_tables_set": (i32, [vp, vp, vp, vp, vp]),
        "scopa_team_cfr_iterate": (i32, [vp, i32, vp, vp]),
        "scopa_team_cfr_traverse": (i32, [vp, i32, C.POINTER(C.c_double)]),
        "scopa_team_cfr_launch": (i32, [vp, i32, i32]),
        "scopa_team_exploitability": (i32, [vp, vp, C.POINTER(C.c_double * 4), vp]),
        "scopa_team_minimax": (i32, [vp, C.POINTER(C.c_double), vp]),
        "scopa_team_policy_value": (i32, [vp, vp, vp, C.POINTER(C.c_double)]),
        "scopa_team_chance_create": (i32, [vp, i32, vp, C.POINTER(vp)]),
        "scopa_team_chance_destroy": (i32, [vp]),
        "scopa_team_chance_debug_image_budget": (i32, [vp, i64]),
        "scopa_team_chance_counts": (i32, [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]),
        "scopa_team_chance_index_get": (i32, [vp, vp, vp]),
        "scopa_team_chance_tables_reset": (i32, [vp]),
        "scopa_team_chance_tables_get": (i32, [vp, vp, vp]),
        "scopa_team_chance_tables_set": (i32, [vp, vp, vp]),
        "scopa_team_chance_sigma_get": (i32, [vp, vp]),
        "scopa_team_chance_cfr_iterate": (i32, [vp, i32, vp, vp]),
        "scopa_team_chance_cfr_iterate_sampled": (i32, [vp, i32, i32, vp, vp, i32, vp]),
        "scopa_team_chance_cfr_launch": (i32, [vp, i32, i32]),
        "scopa_team_chance_exploitability": (i32, [vp, vp, C.POINTER(C.c_double * 4), vp, vp]),
        "scopa_team_chance_policy_for_deal": (i32, [vp, vp, i32, vp]),
        "scopa_team_chance_mccfr_traverse": (i32, [vp, C.c_uint32, i32, C.c_uint32, C.c_uint32]),
        "scopa_team_chance_mccfr_apply": (i32, [vp]),
        "scopa_team_chance_mccfr_walk": (i32, [vp, C.c_uint32, C.c_uint32, i32, vp]),
        "scopa_team_chance_mccfr_iterate": (i32, [vp, i32, C.c_uint32, i32, vp]),
        "scopa_team_chance_mccfr_counters": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
        "scopa_team_chance_mccfr_delta_get": (i32, [vp, vp]),
        "scopa_team_cross_play": (i32, [vp, i32, vp, vp]),
        "scopa_team_match": (i32, [vp, vp, vp, i64, i64, C.c_uint32, vp, vp]),
        "scopa_team_debug_xplay_group_limit": (i32, [vp, i64]),
        "scopa_team_chance_cross_play": (i32, [vp, i32, vp, vp, vp]),
        "scopa_team_chance_match": (i32, [vp, vp, vp, i64, i64, C.c_uint32, vp, vp, vp]),
        "scopa_team_chance_sdcfr_traverse": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, i64, vp, u32, u32]),
        "scopa_team_chance_sdcfr_visits": (i32, [vp, C.POINTER(u64)]),
        "scopa_team_chance_sdcfr_policy_get": (i32, [vp, i32, vp, vp]),
        "scopa_team_chance_sdcfr_forced_get": (i32, [vp, i32, vp]),
        "scopa_team_chance_sdcfr_average_policy": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
        "scopa_team_chance_debug_sdcfr": (i32, [vp, i64, i32, i32]),
        "scopa_team_mccfr_replay": (i32, [vp, i32, vp, i64, C.POINTER(i64)]),
        "scopa_team_mccfr_traverse": (i32, [vp, C.c_uint32, C.c_uint32, C.c_uint32]),
        "scopa_team_mccfr_apply": (i32, [vp]),
        "scopa_team_mccfr_iterate": (i32, [vp, C.c_uint32, C.c_uint32]),
        "scopa_team_mccfr_counters": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
        "scopa_team_mccfr_delta_get": (i32, [vp, vp]),
        "scopa_team_mccfr_visits_get": (i32, [vp, vp, vp]),
        "scopa_counters": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "scopa_prof_enable": (i32, [vp, i32]),
        "scopa_prof_read": (i32, [vp, C.POINTER(i64), C.POINTER(C.c_double)]),
        "scopa_prof_device": (i32, [vp, C.POINTER(i64), C.POINTER(C.c_double)]),
        "scopa_prof_phases": (i32, [vp, C.POINTER(C.c_double * 3)]),
        "scopa_prof_spread": (i32, [vp, C.POINTER(C.c_double * 3)]),
    }
    # A/B tooling only (tests/tools/ab_time.sh): a variant library built from an OLDER revision, named through SCOPA_HIP_LIBRARY, may lack entry points
    # added since -- with SCOPA_AB_OLD_LIBRARY=1 those are left unbound (calling one raises AttributeError); the product's own library must export them all
    lenient = bool(os.environ.get("SCOPA_HIP_LIBRARY")) and os.environ.get("SCOPA_AB_OLD_LIBRARY") == "1"
    for name, (res, args) in sig.items():
        if lenient and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    if L.scopa_abi_version() != 1:
        raise OSError("libscopa_hip.so ABI version mismatch")
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _weights(weights):
    """float64 [n][3] rows of (pos, neg, strat) as the weighted synchronous-CFR calls take them (at least one row allocated: a non-NULL pointer)"""
    w = np.ascontiguousarray(weights, np.float64).reshape(-1, 3)
    return (w if w.size else np.ones((1, 3))), w.shape[0]


def deal_py_seed(seed):
    """16-card permutation of random.seed(seed); random.shuffle(deck) (MiniDeck, mini_scopa_game.py:25-28)."""
    perm = np.zeros(16, np.uint8)
    rc = lib().scopa_deal_py_seed(int(seed), _ptr(perm))
    if rc:
        raise ScopaError(rc, "scopa_deal_py_seed")
    return perm


def key_to_string(key):
    buf = C.create_string_buffer(96)
    rc = lib().scopa_key_to_string(int(key), buf, 96)
    if rc < 0:
        raise ScopaError(rc, "scopa_key_to_string")
    return buf.value.decode()


class Context:
    """One scopa_ctx: a HIP device + stream + (after set_deal) one game tree and its tables."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self._L = lib()
        rc = self._L.scopa_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self._h))
        if rc:
            self._h = None
            raise ScopaError(rc, "scopa_ctx_create", "a GPU is required: the solver path has no CPU fallback")
        self.device = device
        self.stream = stream         # the caller's HIP stream handle, or None: a stream the library created for itself
        self.n_infosets = 0
        self._children = []  # weakrefs of objects that hold device memory through this context (MultiDeal)

    def close(self):
        if getattr(self, "_h", None):
            for ref in getattr(self, "_children", []):
                child = ref()
                if child is not None:
                    child.close()
            self._L.scopa_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, where):
        if rc:
            raise ScopaError(rc, where, self._L.scopa_last_error(self._h).decode())

    def synchronize(self):
        self._ck(self._L.scopa_ctx_synchronize(self._h), "scopa_ctx_synchronize")

    # ---- batched step ---------------------------------------------------------------------
    def step_batch_host(self, states, actions):
        """states: np array of STATE_DTYPE (modified in place), actions: uint8."""
        assert states.dtype == STATE_DTYPE and states.flags.c_contiguous
        actions = np.ascontiguousarray(actions, np.uint8)
        assert actions.size == states.size
        self._ck(self._L.scopa_step_batch_host(self._h, _ptr(states), _ptr(actions), states.size), "scopa_step_batch_host")
        return states

    def step_batch(self, d_states_ptr, d_actions_ptr, n):
        self._ck(self._L.scopa_step_batch(self._h, C.c_void_p(d_states_ptr), C.c_void_p(d_actions_ptr), int(n)), "scopa_step_batch")

    # ---- deal / tree ------------------------------------------------------------------------
    def set_deal(self, perm16):
        perm = np.ascontiguousarray(perm16, np.uint8)
        assert perm.size == 16
        self._ck(self._L.scopa_set_deal(self._h, _ptr(perm)), "scopa_set_deal")
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._L.scopa_tree_counts(self._h, C.byref(a), C.byref(b), C.byref(c)), "scopa_tree_counts")
        self.n_infosets = c.value
        self.perm = perm
        return self.n_infosets

    def tree_export(self):
        I = self.n_infosets
        out = dict(states=np.zeros(N_NODES, STATE_DTYPE), infoset=np.zeros(N_NODES, np.int32), r2=np.zeros((N_NODES, 2), np.int8),
                   infoset_key=np.zeros(I, np.uint64), infoset_nlegal=np.zeros(I, np.int8), infoset_legal=np.zeros((I, 4), np.int8))
        self._ck(self._L.scopa_tree_export(self._h, _ptr(out["states"]), _ptr(out["infoset"]), _ptr(out["r2"]),
                                           _ptr(out["infoset_key"]), _ptr(out["infoset_nlegal"]), _ptr(out["infoset_legal"])),
                 "scopa_tree_export")
        return out

    # ---- tables ------------------------------------------------------------------------------
    def tables_reset(self):
        self._ck(self._L.scopa_tables_reset(self._h), "scopa_tables_reset")

    def tables_get(self, regret=True, strategy=True, local=True):
        I = self.n_infosets
        R = np.zeros((I, 4)) if regret else None
        S = np.zeros((I, 4)) if strategy else None
        Lc = np.zeros((I, 4)) if local else None
        self._ck(self._L.scopa_tables_get(self._h, _ptr(R), _ptr(S), _ptr(Lc)), "scopa_tables_get")
        return R, S, Lc

    def tables_set(self, regret=None, strategy=None, local=None):
        arrs = []
        for a in (regret, strategy, local):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64)
                assert a.shape == (self.n_infosets, 4)
            arrs.append(a)
        self._ck(self._L.scopa_tables_set(self._h, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2])), "scopa_tables_set")

    # ---- solvers ------------------------------------------------------------------------------
    def cfr_exact_iterate(self, n_iters):
        rv = np.zeros((max(int(n_iters), 0), 2))
        self._ck(self._L.scopa_cfr_exact_iterate(self._h, int(n_iters), _ptr(rv)), "scopa_cfr_exact_iterate")
        return rv

    def cfr_exact_mode(self, sequential):
        """False (default): whole-tree traversals as a parallel schedule; True: the one-lane sequential walk.  Same tables bit for bit."""
        self._ck(self._L.scopa_cfr_exact_mode(self._h, 1 if sequential else 0), "scopa_cfr_exact_mode")

    def cfr_exact_last_route(self):
        """the kernel the last exact-CFR call ran: 0 scheduled, 1 one-lane walk with the tables in LDS, 2 the same with the tables in HBM, -1 none yet"""
        r = C.c_int32()
        self._ck(self._L.scopa_cfr_exact_last_route(self._h, C.byref(r)), "scopa_cfr_exact_last_route")
        return r.value

    def cfr_exact_traverse(self, traverser):
        v = C.c_double()
        self._ck(self._L.scopa_cfr_exact_traverse(self._h, int(traverser), C.byref(v)), "scopa_cfr_exact_traverse")
        return v.value

    def cfr_exact_traverse_from(self, traverser, path, reach_p0=1.0, reach_p1=1.0):
        pa = np.ascontiguousarray(path, np.int32)
        v = C.c_double()
        self._ck(self._L.scopa_cfr_exact_traverse_from(self._h, int(traverser), pa.size, _ptr(pa), float(reach_p0), float(reach_p1),
                                                       C.byref(v)), "scopa_cfr_exact_traverse_from")
        return v.value

    def visited_get(self):
        seq = np.zeros(self.n_infosets, np.uint32)
        self._ck(self._L.scopa_visited_get(self._h, _ptr(seq)), "scopa_visited_get")
        return seq

    def mccfr_replay(self, n_iters, uniforms):
        u = np.ascontiguousarray(uniforms, np.float64)
        used = C.c_int64()
        self._ck(self._L.scopa_mccfr_replay(self._h, int(n_iters), _ptr(u), u.size, C.byref(used)), "scopa_mccfr_replay")
        return used.value

    def mccfr_seed(self, seed):
        self._ck(self._L.scopa_mccfr_seed(self._h, int(seed)), "scopa_mccfr_seed")

    def mccfr_iterate(self, batch, n_iters):
        self._ck(self._L.scopa_mccfr_iterate(self._h, int(batch), int(n_iters)), "scopa_mccfr_iterate")

    def mccfr_traverse(self, iteration, b0, nb):
        self._ck(self._L.scopa_mccfr_traverse(self._h, int(iteration), int(b0), int(nb)), "scopa_mccfr_traverse")

    def mccfr_delta_buffer(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self._L.scopa_mccfr_delta_buffer(self._h, C.byref(p), C.byref(n)), "scopa_mccfr_delta_buffer")
        return p.value, n.value

    def mccfr_bind_delta(self, d_ptr, nbytes):
        """Use a caller-owned device buffer (e.g. torch tensor .data_ptr()) as the all-reduce payload."""
        self._ck(self._L.scopa_mccfr_bind_delta(self._h, C.c_void_p(d_ptr) if d_ptr else None, int(nbytes)), "scopa_mccfr_bind_delta")

    def mccfr_delta_get(self):
        d = np.zeros((self.n_infosets, 5))
        self._ck(self._L.scopa_mccfr_delta_get(self._h, _ptr(d)), "scopa_mccfr_delta_get")
        return d

    def mccfr_delta_set(self, d):
        d = np.ascontiguousarray(d, np.float64)
        assert d.shape == (self.n_infosets, 5)
        self._ck(self._L.scopa_mccfr_delta_set(self._h, _ptr(d)), "scopa_mccfr_delta_set")

    def mccfr_apply(self):
        self._ck(self._L.scopa_mccfr_apply(self._h), "scopa_mccfr_apply")

    def mccfr_graph_mode(self, on):
        """replay scopa_mccfr_iterate's (traverse, apply) launches as captured HIP graphs of up to 64 iterations (same results)"""
        self._ck(self._L.scopa_mccfr_graph_mode(self._h, 1 if on else 0), "scopa_mccfr_graph_mode")

    def debug_lds_limit(self, nbytes):
        self._ck(self._L.scopa_debug_lds_limit(self._h, int(nbytes)), "scopa_debug_lds_limit")

    def mccfr_iteration(self):
        v = C.c_uint32()
        self._ck(self._L.scopa_mccfr_iteration_counter(self._h, C.byref(v)), "scopa_mccfr_iteration_counter")
        return v.value

    def exploitability(self, policy=None, return_policy=False):
        """-> dict(exploitability, br0, br1, value_p0[, policy]); policy=None evaluates the average policy."""
        pin = None if policy is None else np.ascontiguousarray(policy, np.float64)
        out = np.zeros(4)
        pout = np.zeros((self.n_infosets, 4)) if return_policy else None
        self._ck(self._L.scopa_exploitability(self._h, _ptr(pin), _ptr(out), _ptr(pout)), "scopa_exploitability")
        res = dict(exploitability=out[0], br0=out[1], br1=out[2], value_p0=out[3])
        if return_policy:
            res["policy"] = pout
        return res

    # ---- SDCFR / evaluation building blocks (device pointers: torch tensors' data_ptr()) --------------
    def sdcfr_features(self, ply, n, idx_ptr, feats_ptr, mask_ptr):
        self._ck(self._L.scopa_sdcfr_features(self._h, ply, n, C.c_void_p(idx_ptr), C.c_void_p(feats_ptr), C.c_void_p(mask_ptr)), "scopa_sdcfr_features")

    def sdcfr_expand(self, ply, traverser, n, idx_ptr, adv_ptr, child_ptr, pol_ptr, uniforms_ptr, iteration, b0):
        self._ck(self._L.scopa_sdcfr_expand(self._h, ply, traverser, n, C.c_void_p(idx_ptr), C.c_void_p(adv_ptr), C.c_void_p(child_ptr),
                                            C.c_void_p(pol_ptr), C.c_void_p(uniforms_ptr) if uniforms_ptr else None, iteration, b0), "scopa_sdcfr_expand")

    def sdcfr_terminal_values(self, traverser, n, idx_ptr, val_ptr):
        self._ck(self._L.scopa_sdcfr_terminal_values(self._h, traverser, n, C.c_void_p(idx_ptr), C.c_void_p(val_ptr)), "scopa_sdcfr_terminal_values")

    def sdcfr_backward(self, ply, traverser, n, idx_ptr, pol_ptr, child_val_ptr, val_ptr, feats_ptr, mask_ptr, mem_feat_ptr, mem_regret_ptr,
                       mem_mask_ptr, capacity, write_base):
        vp = lambda x: C.c_void_p(x) if x else None
        self._ck(self._L.scopa_sdcfr_backward(self._h, ply, traverser, n, vp(idx_ptr), vp(pol_ptr), vp(child_val_ptr), vp(val_ptr), vp(feats_ptr),
                                              vp(mask_ptr), vp(mem_feat_ptr), vp(mem_regret_ptr), vp(mem_mask_ptr), capacity, write_base),
                 "scopa_sdcfr_backward")

    def sdcfr_pack_weights(self, player, w1_ptr, b1_ptr, w2_ptr, b2_ptr, w3_ptr, b3_ptr, image_ptr):
        """torch tensors of one advantage net (W[out][in], float32) -> `player`'s half of the fused kernel's weight image."""
        self._ck(self._L.scopa_sdcfr_pack_weights(self._h, player, *(C.c_void_p(x) for x in (w1_ptr, b1_ptr, w2_ptr, b2_ptr, w3_ptr, b3_ptr, image_ptr))),
                 "scopa_sdcfr_pack_weights")

    def sdcfr_mode(self, forward_per_visit):
        """0 = policy table per launch + walks (default), 1 = a forward pass per visit inside the traversal kernel; same results"""
        self._ck(self._L.scopa_sdcfr_mode(self._h, 1 if forward_per_visit else 0), "scopa_sdcfr_mode")

    def sdcfr_tuning(self, traversals_per_task=0, wavefronts_per_task=0):
        """only (0, 0), the library's one task shape, is accepted: the other shapes are retired (ScopaError, SCOPA_EINVAL)"""
        self._ck(self._L.scopa_sdcfr_tuning(self._h, traversals_per_task, wavefronts_per_task), "scopa_sdcfr_tuning")

    def sdcfr_train_steps(self, rows_ptr, n_rows, n_steps, feat_ptr, regret_ptr, mask_ptr, capacity, param_ptrs, state_ptr, first_step, lr, loss_ptr):
        """n_steps consecutive optimiser steps (the epochs of one train() call) on rows [n_steps][n_rows]"""
        self._ck(self._L.scopa_sdcfr_train_steps(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_steps), C.c_void_p(feat_ptr), C.c_void_p(regret_ptr), C.c_void_p(mask_ptr),
                                                 int(capacity), *(C.c_void_p(p) for p in param_ptrs), C.c_void_p(state_ptr), int(first_step), float(lr),
                                                 C.c_void_p(loss_ptr)), "scopa_sdcfr_train_steps")

    def full_sdcfr_train_steps(self, rows_ptr, n_rows, n_steps, feat_ptr, regret_ptr, mask_ptr, capacity, param_ptrs, state_ptr, first_step, lr, loss_ptr):
        """the same for FullScopa's 96-128-64-40 net (three launches per step): features [capacity][96], regrets and masks [capacity][40], state [2][23272]"""
        self._ck(self._L.scopa_full_sdcfr_train_steps(self._h, C.c_void_p(rows_ptr), int(n_rows), int(n_steps), C.c_void_p(feat_ptr), C.c_void_p(regret_ptr), C.c_void_p(mask_ptr),
                                                      int(capacity), *(C.c_void_p(p) for p in param_ptrs), C.c_void_p(state_ptr), int(first_step), float(lr),
                                                      C.c_void_p(loss_ptr)), "scopa_full_sdcfr_train_steps")

    def sdcfr_train_step(self, rows_ptr, n_rows, feat_ptr, regret_ptr, mask_ptr, capacity, param_ptrs, state_ptr, step, lr, loss_ptr):
        """one optimiser step of an advantage net in two HIP launches (include/scopa.h); param_ptrs = (w1, b1, w2, b2, w3, b3) device pointers"""
        self._ck(self._L.scopa_sdcfr_train_step(self._h, C.c_void_p(rows_ptr), int(n_rows), C.c_void_p(feat_ptr), C.c_void_p(regret_ptr), C.c_void_p(mask_ptr),
                                                int(capacity), *(C.c_void_p(p) for p in param_ptrs), C.c_void_p(state_ptr), int(step), float(lr),
                                                C.c_void_p(loss_ptr)), "scopa_sdcfr_train_step")

    def sdcfr_traverse_fused(self, traverser, batch, weights_ptr, mem_feat_ptr, mem_regret_ptr, mem_mask_ptr, capacity, write_base,
                             root_values_ptr, uniforms_ptr, iteration, b0):
        self._ck(self._L.scopa_sdcfr_traverse_fused(self._h, traverser, batch, C.c_void_p(weights_ptr), C.c_void_p(mem_feat_ptr),
                                                    C.c_void_p(mem_regret_ptr), C.c_void_p(mem_mask_ptr), capacity, write_base,
                                                    C.c_void_p(root_values_ptr), C.c_void_p(uniforms_ptr) if uniforms_ptr else None,
                                                    iteration, b0), "scopa_sdcfr_traverse_fused")

    def sdcfr_average_policy(self, player, n_snap, param_ptrs, max_size, slots_ptr, coef_ptr, policy_ptr):
        """the rows of `player`'s infosets in the [n_infosets][4] float64 device table at policy_ptr: the average policy of n_snap snapshots of a
        StrategyBuffer store (param_ptrs = (w1, b1, w2, b2, w3, b3) [max_size][...] device pointers, slots / coefficients int32 / float32 [n_snap])"""
        vp = lambda x: C.c_void_p(x) if x else None
        self._ck(self._L.scopa_sdcfr_average_policy(self._h, int(player), int(n_snap), *(vp(p) for p in param_ptrs), int(max_size), vp(slots_ptr),
                                                    vp(coef_ptr), vp(policy_ptr)), "scopa_sdcfr_average_policy")

    def sdcfr_visits(self):
        v = C.c_uint64()
        self._ck(self._L.scopa_sdcfr_visits(self._h, C.byref(v)), "scopa_sdcfr_visits")
        return v.value

    def sdcfr_policy_get(self):
        """(policy [1653][4] float32, thresholds [1653][3] uint64) of the last policy-table launch (include/scopa.h: scopa_sdcfr_policy_get)"""
        pol, thr = np.zeros((N_DECISION, 4), np.float32), np.zeros((N_DECISION, 3), np.uint64)
        self._ck(self._L.scopa_sdcfr_policy_get(self._h, _ptr(pol), _ptr(thr)), "scopa_sdcfr_policy_get")
        return pol, thr

    def features_from_states(self, states_ptr, n, feats_ptr, mask_ptr):
        self._ck(self._L.scopa_features_from_states(self._h, C.c_void_p(states_ptr), n, C.c_void_p(feats_ptr), C.c_void_p(mask_ptr)), "scopa_features_from_states")

    def eval_init_states(self, states_ptr, n):
        self._ck(self._L.scopa_eval_init_states(self._h, C.c_void_p(states_ptr), n), "scopa_eval_init_states")

    def eval_step(self, states_ptr, n, probs_ptr, seat_ptr, stream_id, ply_tag):
        self._ck(self._L.scopa_eval_step(self._h, C.c_void_p(states_ptr), n, C.c_void_p(probs_ptr) if probs_ptr else None, C.c_void_p(seat_ptr),
                                         stream_id, ply_tag), "scopa_eval_step")

    def eval_tabular_prepare(self, policy_ptr):
        """sampling thresholds of a tabular policy, once per evaluation; eval_tabular_step(..., policy_ptr=0, ...) then uses them"""
        self._ck(self._L.scopa_eval_tabular_prepare(self._h, C.c_void_p(policy_ptr)), "scopa_eval_tabular_prepare")

    def eval_tabular_step(self, states_ptr, idx_ptr, n, ply, policy_ptr, seat_ptr, stream_id):
        self._ck(self._L.scopa_eval_tabular_step(self._h, C.c_void_p(states_ptr), C.c_void_p(idx_ptr), n, ply, C.c_void_p(policy_ptr) if policy_ptr else None,
                                                 C.c_void_p(seat_ptr), stream_id), "scopa_eval_tabular_step")

    def eval_tabular_match(self, n, n_seat0, stream_id, states_ptr=0, idx_ptr=0):
        """the whole match of the prepared policy vs uniform random in one launch -> int64 [2][5]: per seat half (episodes, sum r x2, sum (r x2)^2,
        sum trained scopas, sum opponent scopas); optionally the final states / terminal indices into device buffers"""
        st = np.zeros((2, 5), np.int64)
        self._ck(self._L.scopa_eval_tabular_match(self._h, int(n), int(n_seat0), stream_id, C.c_void_p(states_ptr) if states_ptr else None,
                                                  C.c_void_p(idx_ptr) if idx_ptr else None, _ptr(st)), "scopa_eval_tabular_match")
        return st

    def cross_play(self, n_pol, policies_ptr, out_ptr):
        """device pointers: policies [n_pol][n_infosets][4] float64 -> out [n_pol][n_pol][4] float64, out[a][b] = exact (reward of seat 0, its square,
        scopas of seat 0, scopas of seat 1) of policy a in seat 0 against policy b in seat 1; one launch on the context's stream, no synchronisation"""
        self._ck(self._L.scopa_cross_play(self._h, int(n_pol), C.c_void_p(policies_ptr) if policies_ptr else None, C.c_void_p(out_ptr) if out_ptr else None),
                 "scopa_cross_play")

    def best_response(self, n_pol, policies_ptr, br_ptr, out4_ptr):
        """device pointers: policies [n_pol][n_infosets][4] -> out4 [n_pol][4] = (exploitability, BR0, BR1, value) as scopa_exploitability gives them, and
        (br_ptr, or 0) br [n_pol][2][n_infosets][4]: the best-response tables themselves; on the context's stream, no synchronisation"""
        self._ck(self._L.scopa_best_response(self._h, int(n_pol), C.c_void_p(policies_ptr) if policies_ptr else None, C.c_void_p(br_ptr) if br_ptr else None,
                                             C.c_void_p(out4_ptr) if out4_ptr else None), "scopa_best_response")

    def eval_pair_match(self, policy_a_ptr, policy_b_ptr, n, n_seat0, stream_id, idx_ptr=0):
        """eval_tabular_match with a policy in both seats (device pointers to two [n_infosets][4] float64 tables; episodes i < n_seat0 have a in seat 0)
        -> int64 [2][5] per seat half, from a's point of view; optionally every episode's terminal index into a device buffer"""
        st = np.zeros((2, 5), np.int64)
        self._ck(self._L.scopa_eval_pair_match(self._h, C.c_void_p(policy_a_ptr) if policy_a_ptr else None, C.c_void_p(policy_b_ptr) if policy_b_ptr else None,
                                               int(n), int(n_seat0), stream_id, C.c_void_p(idx_ptr) if idx_ptr else None, _ptr(st)), "scopa_eval_pair_match")
        return st

    def cfr_sync_iterate(self, n_iters):
        self._ck(self._L.scopa_cfr_sync_iterate(self._h, int(n_iters)), "scopa_cfr_sync_iterate")

    def cfr_sync_iterate_weighted(self, weights, alternating=False):
        """one synchronous-CFR iteration per row (pos, neg, strat) of `weights` (scopa_amd.algorithms.cfr_variants.schedule builds them)"""
        w, n = _weights(weights)
        self._ck(self._L.scopa_cfr_sync_iterate_weighted(self._h, n, _ptr(w), int(alternating)), "scopa_cfr_sync_iterate_weighted")

    def full_step_batch_host(self, states, actions, decks):
        assert states.dtype == FULL_STATE_DTYPE
        actions = np.ascontiguousarray(actions, np.uint8)
        decks = np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        self._ck(self._L.scopa_full_step_batch_host(self._h, _ptr(states), _ptr(actions), _ptr(decks), decks.shape[0], states.size),
                 "scopa_full_step_batch_host")
        return states

    def full_step_batch(self, states_ptr, actions_ptr, decks_ptr, n):
        """device pointers: states[n] (64 B each) <- step(states[i], decks[states[i].game], actions[i])"""
        self._ck(self._L.scopa_full_step_batch(self._h, C.c_void_p(states_ptr), C.c_void_p(actions_ptr), C.c_void_p(decks_ptr), int(n)), "scopa_full_step_batch")

    def full_random_playouts(self, seeds):
        seeds = np.ascontiguousarray(seeds, np.int64)
        r2, plies = np.zeros(seeds.size, np.int8), np.zeros(seeds.size, np.int16)
        self._ck(self._L.scopa_full_random_playouts(self._h, _ptr(seeds), seeds.size, _ptr(r2), _ptr(plies)), "scopa_full_random_playouts")
        return r2, plies

    def p2p_create(self, rank, world):
        """-> this rank's 64-byte IPC handle (uint8[64]) of its peer-exchange inbox"""
        h = np.zeros(64, np.uint8)
        self._ck(self._L.scopa_p2p_create(self._h, int(rank), int(world), _ptr(h)), "scopa_p2p_create")
        return h

    def p2p_connect(self, handles):
        handles = np.ascontiguousarray(handles, np.uint8).reshape(-1, 64)
        self._ck(self._L.scopa_p2p_connect(self._h, _ptr(handles)), "scopa_p2p_connect")

    def p2p_allreduce_delta(self):
        self._ck(self._L.scopa_p2p_allreduce_delta(self._h), "scopa_p2p_allreduce_delta")

    def mccfr_iterate_sharded(self, b0, nb, n_iters=1):
        self._ck(self._L.scopa_mccfr_iterate_sharded(self._h, int(b0), int(nb), int(n_iters)), "scopa_mccfr_iterate_sharded")

    def p2p_status(self):
        """-> (waits that timed out, exchanges issued); synchronises the stream"""
        t, n = C.c_int32(), C.c_uint64()
        self._ck(self._L.scopa_p2p_status(self._h, C.byref(t), C.byref(n)), "scopa_p2p_status")
        return t.value, n.value

    def p2p_set_form(self, light):
        """False (default): plain accesses + system-scope fences; True: sc0 sc1 accesses ordered by s_waitcnt (validate first)"""
        self._ck(self._L.scopa_p2p_set_form(self._h, 1 if light else 0), "scopa_p2p_set_form")

    def p2p_set_budget(self, seconds):
        self._ck(self._L.scopa_p2p_set_budget(self._h, float(seconds)), "scopa_p2p_set_budget")

    def p2p_destroy(self):
        self._ck(self._L.scopa_p2p_destroy(self._h), "scopa_p2p_destroy")

    def team_step_batch_host(self, states, actions):
        assert states.dtype == TEAM_STATE_DTYPE
        actions = np.ascontiguousarray(actions, np.uint8)
        self._ck(self._L.scopa_team_step_batch_host(self._h, _ptr(states), _ptr(actions), states.size), "scopa_team_step_batch_host")
        return states

    def team_step_batch(self, states_ptr, actions_ptr, n):
        """device pointers: states[n] (40 B each) <- step(states[i], actions[i])"""
        self._ck(self._L.scopa_team_step_batch(self._h, C.c_void_p(states_ptr), C.c_void_p(actions_ptr), int(n)), "scopa_team_step_batch")

    def team_random_playouts(self, seeds):
        """-> (reward x2 of team 0 per game, scopas[n][4] per seat)"""
        seeds = np.ascontiguousarray(seeds, np.int64)
        r2, sc = np.zeros(seeds.size, np.int8), np.zeros((seeds.size, 4), np.uint8)
        self._ck(self._L.scopa_team_random_playouts(self._h, _ptr(seeds), seeds.size, _ptr(r2), _ptr(sc)), "scopa_team_random_playouts")
        return r2, sc

    # ---- Team MiniScopa solved for one fixed deal (scopa_team_cfr.hip) ---------------------------
    def team_set_deal(self, perm16):
        perm = np.ascontiguousarray(perm16, np.uint8)
        assert perm.size == 16
        self._ck(self._L.scopa_team_set_deal(self._h, _ptr(perm)), "scopa_team_set_deal")
        self.team_perm = perm

    def team_tree_counts(self):
        """-> (choice nodes, depth-12 nodes, infosets)"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._L.scopa_team_tree_counts(self._h, C.byref(a), C.byref(b), C.byref(c)), "scopa_team_tree_counts")
        return a.value, b.value, c.value

    def team_tree_leaves(self):
        r2 = np.zeros(TEAM_N_LEAVES, np.int8)
        self._ck(self._L.scopa_team_tree_leaves(self._h, _ptr(r2)), "scopa_team_tree_leaves")
        return r2

    def team_tables_reset(self):
        self._ck(self._L.scopa_team_tables_reset(self._h), "scopa_team_tables_reset")

    def team_tables_get(self, regret=True, strategy=True, local=True, leaf_reach=True):
        """-> (regret, strategy, local) [TEAM_N_CHOICE][4] and leaf_reach_sum [2][TEAM_N_LEAVES]; None for a table not asked for"""
        R, S, Lc = (np.zeros((TEAM_N_CHOICE, 4)) if want else None for want in (regret, strategy, local))
        Q = np.zeros((2, TEAM_N_LEAVES)) if leaf_reach else None
        self._ck(self._L.scopa_team_tables_get(self._h, _ptr(R), _ptr(S), _ptr(Lc), _ptr(Q)), "scopa_team_tables_get")
        return R, S, Lc, Q

    def team_tables_set(self, regret=None, strategy=None, local=None, leaf_reach=None):
        arrs = []
        for a, shape in ((regret, (TEAM_N_CHOICE, 4)), (strategy, (TEAM_N_CHOICE, 4)), (local, (TEAM_N_CHOICE, 4)), (leaf_reach, (2, TEAM_N_LEAVES))):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64)
                assert a.shape == shape
            arrs.append(a)
        self._ck(self._L.scopa_team_tables_set(self._h, *(_ptr(a) for a in arrs)), "scopa_team_tables_set")

    def team_cfr_iterate(self, n_iters, weights=None, root_values=True):
        """n_iters iterations; weights: None (the reference) or [n_iters][3] rows of (pos, neg, strat).  -> root values [n_iters][2], or None"""
        n_iters = int(n_iters)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float64).reshape(-1, 3)
            assert w.shape[0] == n_iters
            if not w.size:
                w = None
        rv = np.zeros((max(n_iters, 0), 2)) if root_values else None
        self._ck(self._L.scopa_team_cfr_iterate(self._h, n_iters, _ptr(w), _ptr(rv) if root_values and n_iters > 0 else None), "scopa_team_cfr_iterate")
        return rv

    def team_cfr_traverse(self, traverser):
        """one unweighted traversal of `traverser` from the root -> its value"""
        v = C.c_double()
        self._ck(self._L.scopa_team_cfr_traverse(self._h, int(traverser), C.byref(v)), "scopa_team_cfr_traverse")
        return v.value

    def team_cfr_launch(self, traverser, part):
        """one launch of an unweighted traversal (part 0: the subtrees, 1: the top), for timing"""
        self._ck(self._L.scopa_team_cfr_launch(self._h, int(traverser), int(part)), "scopa_team_cfr_launch")

    def team_exploitability(self, policy_ptr=0, br_ptr=0):
        """-> [(BR0 + BR1) / 2, BR0, BR1, value for team 0]; policy_ptr 0 = the average policy; device pointers"""
        out = (C.c_double * 4)()
        self._ck(self._L.scopa_team_exploitability(self._h, C.c_void_p(policy_ptr or None), C.byref(out), C.c_void_p(br_ptr or None)), "scopa_team_exploitability")
        return np.array(out[:])

    def team_minimax(self, policy_out_ptr=0):
        v = C.c_double()
        self._ck(self._L.scopa_team_minimax(self._h, C.byref(v), C.c_void_p(policy_out_ptr or None)), "scopa_team_minimax")
        return v.value

    def team_policy_value(self, policy_a_ptr=0, policy_b_ptr=0):
        v = C.c_double()
        self._ck(self._L.scopa_team_policy_value(self._h, C.c_void_p(policy_a_ptr or None), C.c_void_p(policy_b_ptr or None), C.byref(v)), "scopa_team_policy_value")
        return v.value

    # ---- Team MiniScopa, policy against policy on the context's deal (scopa_team_xplay.hip) --------
    def team_cross_play(self, n_pol, policies_ptr, out_ptr):
        """device pointers: policies [n_pol][TEAM_N_CHOICE][4] float64 -> out [n_pol][n_pol][4], out[a][b] = exact (reward of team 0, its square,
        scopas of team 0, scopas of team 1) of table a as team 0 against table b as team 1; two launches on the context's stream, no synchronisation"""
        vp = lambda x: C.c_void_p(x) if x else None
        self._ck(self._L.scopa_team_cross_play(self._h, int(n_pol), vp(policies_ptr), vp(out_ptr)), "scopa_team_cross_play")

    def team_match(self, policy_a_ptr, policy_b_ptr, n, n_team0, stream_id, leaf_ptr=0):
        """the sampled seat-swapped match of two [TEAM_N_CHOICE][4] float64 device tables: episodes i < n_team0 have a as team 0 -> int64 [2][5] per
        half (episodes, sum of a's rewards x2, sum of their squares, a's team's scopas, b's team's scopas); optionally every episode's depth-12
        index into an int32 device buffer.  The Philox key is mccfr_seed's"""
        vp = lambda x: C.c_void_p(x) if x else None
        st = np.zeros((2, 5), np.int64)
        self._ck(self._L.scopa_team_match(self._h, vp(policy_a_ptr), vp(policy_b_ptr), int(n), int(n_team0), stream_id, vp(leaf_ptr), _ptr(st)), "scopa_team_match")
        return st

    def full_chance_sdcfr_policy_at(self, player, keys_ptr, n, weight_ptrs, policy_ptr, thr_ptr):
        """scopa_full_chance_sdcfr_policy_at: policy [n][3] float32 and thresholds [n][2] uint64 of the n key pairs [n][2] at keys_ptr, all of mover
        `player`, under that player's net of weight_ptrs (six device pointers to [2][...]); device pointers, queued on the context's stream"""
        vp = lambda x: C.c_void_p(x) if x else None
        self._ck(self._L.scopa_full_chance_sdcfr_policy_at(self._h, int(player), vp(keys_ptr), int(n), *(vp(p) for p in weight_ptrs), vp(policy_ptr), vp(thr_ptr)),
                 "scopa_full_chance_sdcfr_policy_at")

    def full_chance_sdcfr_average_at(self, player, keys_ptr, n, slots, param_ptrs, max_size, coef_ptr, policy_ptr):
        """scopa_full_chance_sdcfr_average_at: the average policy [n][3] float64 (device, at policy_ptr) of the snapshots `slots` (FIFO order; indices
        into six device tensors [max_size][...] at param_ptrs) with the float32 coefficients at coef_ptr, at the n key pairs [n][2] at keys_ptr, all of
        mover `player`; ONE launch whatever the snapshot count, queued on the context's stream"""
        vp = lambda x: C.c_void_p(x) if x else None
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        self._ck(self._L.scopa_full_chance_sdcfr_average_at(self._h, int(player), vp(keys_ptr), int(n), slots.size, *(vp(p) for p in param_ptrs),
                                                            _ptr(slots) if slots.size else None, int(max_size), vp(coef_ptr), vp(policy_ptr)),
                 "scopa_full_chance_sdcfr_average_at")

    def full_chance_debug_sdcfr_average_grid(self, workgroups=0):
        """test and benchmark hook: the workgroups of every average_at launch on this context, at most one per tile (0 restores the library's rule)"""
        self._ck(self._L.scopa_full_chance_debug_sdcfr_average_grid(self._h, int(workgroups)), "scopa_full_chance_debug_sdcfr_average_grid")

    def full_chance_debug_sdcfr_scratch(self, nbytes=0):
        """test hook: the bytes a chunk of FullChanceMCCFR.sdcfr_traverse_frontier's traversals may take on this context (0 restores 1 GiB)"""
        self._ck(self._L.scopa_full_chance_debug_sdcfr_scratch(self._h, int(nbytes)), "scopa_full_chance_debug_sdcfr_scratch")

    def team_debug_xplay_group_limit(self, groups):
        """test hook: the workgroup limit of the team cross-play launches on this context (0 restores 2^31)"""
        self._ck(self._L.scopa_team_debug_xplay_group_limit(self._h, int(groups)), "scopa_team_debug_xplay_group_limit")

    # ---- Team MiniScopa, external-sampling MCCFR (scopa_team_mccfr.hip) ----------------------------
    def team_chance_debug_image_budget(self, nbytes):
        """test hook: the byte budget of a TeamChanceGame's increment image for later creates on this context (0 restores the default)"""
        self._ck(self._L.scopa_team_chance_debug_image_budget(self._h, int(nbytes)), "scopa_team_chance_debug_image_budget")

    def team_mccfr_replay(self, n_iters, uniforms):
        """MCCFRTrainer.iteration() n_iters times from the uniforms np.random.choice would draw (TEAM_MCCFR_DRAWS each) -> uniforms consumed"""
        u = np.ascontiguousarray(uniforms, np.float64)
        used = C.c_int64()
        self._ck(self._L.scopa_team_mccfr_replay(self._h, int(n_iters), _ptr(u), u.size, C.byref(used)), "scopa_team_mccfr_replay")
        return used.value

    def team_mccfr_traverse(self, iteration, b0, nb):
        self._ck(self._L.scopa_team_mccfr_traverse(self._h, int(iteration), int(b0), int(nb)), "scopa_team_mccfr_traverse")

    def team_mccfr_apply(self):
        self._ck(self._L.scopa_team_mccfr_apply(self._h), "scopa_team_mccfr_apply")

    def team_mccfr_iterate(self, batch, n_iters):
        self._ck(self._L.scopa_team_mccfr_iterate(self._h, int(batch), int(n_iters)), "scopa_team_mccfr_iterate")

    def team_mccfr_counters(self):
        """-> (decision visits, terminal visits, iterations applied) of the team game's sampling solver"""
        a, b, it = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._ck(self._L.scopa_team_mccfr_counters(self._h, C.byref(a), C.byref(b), C.byref(it)), "scopa_team_mccfr_counters")
        return a.value, b.value, it.value

    def team_mccfr_delta_get(self):
        d = np.zeros((TEAM_N_CHOICE, 5))
        self._ck(self._L.scopa_team_mccfr_delta_get(self._h, _ptr(d)), "scopa_team_mccfr_delta_get")
        return d

    def team_mccfr_visits_get(self):
        """-> seen [TEAM_N_CHOICE] uint8, leaf_visits [2][TEAM_N_LEAVES] uint64"""
        seen, lv = np.zeros(TEAM_N_CHOICE, np.uint8), np.zeros((2, TEAM_N_LEAVES), np.uint64)
        self._ck(self._L.scopa_team_mccfr_visits_get(self._h, _ptr(seen), _ptr(lv)), "scopa_team_mccfr_visits_get")
        return seen, lv

    def counters(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.scopa_counters(self._h, C.byref(a), C.byref(b)), "scopa_counters")
        return a.value, b.value

    def prof_enable(self, stride=1):
        """stride: bracket every stride-th traversal launch with HIP events (True = 1, False/0 = off)."""
        self._ck(self._L.scopa_prof_enable(self._h, int(stride)), "scopa_prof_enable")

    def prof_read(self):
        n, ms = C.c_int64(), C.c_double()
        self._ck(self._L.scopa_prof_read(self._h, C.byref(n), C.byref(ms)), "scopa_prof_read")
        return n.value, ms.value

    def prof_phases(self):
        """after prof_device(): mean us per workgroup of the sampled launches in (prologue, walks, epilogue)"""
        out = (C.c_double * 3)()
        self._ck(self._L.scopa_prof_phases(self._h, C.byref(out)), "scopa_prof_phases")
        return tuple(out)

    def prof_spread(self):
        """(mean workgroup start behind the launch's first, last workgroup's start behind the first, longest workgroup) in us; after prof_device()."""
        out = (C.c_double * 3)()
        self._ck(self._L.scopa_prof_spread(self._h, C.byref(out)), "scopa_prof_spread")
        return [out[0], out[1], out[2]]

    def prof_device(self):
        """-> (traversal launches, their summed milliseconds by the kernel's own 100 MHz clock) since the context was created"""
        n, ms = C.c_int64(), C.c_double()
        self._ck(self._L.scopa_prof_device(self._h, C.byref(n), C.byref(ms)), "scopa_prof_device")
        return n.value, ms.value


FULL_STATE_DTYPE = np.dtype([("table", "<u8", (2,)), ("cap", "<u8", (2,)), ("hand", "<u4", (2,)), ("game", "<u4"), ("nh", "u1", (2,)),
                             ("nt", "u1"), ("deck_pos", "u1"), ("round", "u1"), ("last_capture", "u1"), ("scopas", "u1", (2,)),
                             ("step", "<u2"), ("terminal", "u1"), ("r2_p0", "i1"), ("flags", "u1"), ("pad", "u1", (7,))])
assert FULL_STATE_DTYPE.itemsize == 64


def full_deal_py_seed(seed):
    """40-card FullDeck(seed).cards as card ids (full_scopa_game.py:29-32)."""
    perm = np.zeros(40, np.uint8)
    rc = lib().scopa_full_deal_py_seed(int(seed), _ptr(perm))
    if rc:
        raise ScopaError(rc, "scopa_full_deal_py_seed")
    return perm


class FullState:
    """One packed FullScopa state driven through the host-side protocol (scopa_full_state_*)."""

    def __init__(self, seed=42, deck=None, game=0):
        self.deck = np.ascontiguousarray(full_deal_py_seed(seed) if deck is None else deck, np.uint8)
        self.s = np.zeros(1, FULL_STATE_DTYPE)
        rc = lib().scopa_full_state_init(_ptr(self.deck), int(game), _ptr(self.s))
        if rc:
            raise ScopaError(rc, "scopa_full_state_init")

    def step(self, action):
        rc = lib().scopa_full_state_step(_ptr(self.s), _ptr(self.deck), int(action))
        if rc:
            raise ScopaError(rc, "scopa_full_state_step")

    def legal(self, player=-1):
        out, n = (C.c_int32 * 3)(), C.c_int32()
        lib().scopa_full_state_legal(_ptr(self.s), int(player), C.byref(out), C.byref(n))
        return [out[i] for i in range(n.value)]

    def is_terminal(self):
        return bool(self.s[0]["terminal"])

    def current_player(self):
        return -4 if self.is_terminal() else int(self.s[0]["step"]) & 1

    def rewards(self):
        r = int(self.s[0]["r2_p0"])
        return [r / 2.0, -r / 2.0] if self.is_terminal() else [0, 0]

    def infoset_string(self, player):
        buf = C.create_string_buffer(256)
        lib().scopa_full_state_infoset_string(_ptr(self.s), int(player), buf, 256)
        return buf.value.decode()

    def snapshot(self):
        return unpack_full_state(self.s[0])


def full_infoset_key(state, deck, player):
    """scopa_full_infoset_key of a FULL_STATE_DTYPE record (or a FullState) on its deck: host code, no GPU"""
    s = state.s if isinstance(state, FullState) else np.ascontiguousarray(state, FULL_STATE_DTYPE).reshape(1)
    key = C.c_uint64()
    rc = lib().scopa_full_infoset_key(_ptr(s), _ptr(np.ascontiguousarray(deck, np.uint8)), int(player), C.byref(key))
    if rc:
        raise ScopaError(rc, "scopa_full_infoset_key")
    return key.value


_FULL_SUITS = ("denari", "coppe", "spade", "bastoni")


def full_key_fields(key, deck):
    """a key of scopa_full_infoset_key on `deck` -> dict(player, round, hand (cards in deal order = action slots), table (cards, ascending id), ncap
    [player 0, player 1], scopas): everything scopa_full_state_infoset_string says, the opponent's capture count from the cards dealt so far"""
    key = int(key)
    player, rnd, sub = (key >> 62) & 1, (key >> 59) & 7, (key >> 56) & 7
    hand = [int(deck[4 + 6 * rnd + 3 * player + i]) for i in range(3) if (sub >> i) & 1]
    table = [c for c in range(40) if (key >> (16 + c)) & 1]
    own = (key >> 10) & 63
    other = 4 + 6 * (rnd + 1) - len(table) - 2 * len(hand) + player - own       # the opponent holds as many cards (player 0 to move) or one fewer
    return dict(player=player, round=rnd, hand=hand, table=table, ncap=[other, own] if player else [own, other], scopas=[(key >> 5) & 31, key & 31])


def full_key_to_string(key, deck):
    """information_state_string (openspiel_full_scopa.py:79-94) of the decision node a key stands for on `deck`"""
    f = full_key_fields(key, deck)
    name = lambda cards: "-".join(f"{c % 10 + 1}{_FULL_SUITS[c // 10][0]}" for c in sorted(cards, key=lambda c: (c % 10 + 1, _FULL_SUITS[c // 10])))
    return (f"P{f['player']}:R{f['round']}:H[{name(f['hand'])}]:T[{name(f['table'])}]:C[{f['ncap'][0]},{f['ncap'][1]}]"
            f":S[{f['scopas'][0]},{f['scopas'][1]}]")


class FullMCCFR:
    """One scopa_full_mccfr: the keyed store of FullScopa infoset rows on `ctx`'s device and the sampling solver over it (include/scopa.h)."""

    def __init__(self, ctx, deck, root=None, capacity_log2=22):
        import weakref
        self._h, self._ctx, self._L = C.c_void_p(), ctx, lib()
        self.deck = np.ascontiguousarray(deck, np.uint8)
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        rc = self._L.scopa_full_mccfr_create(ctx._h, _ptr(self.deck), _ptr(root), int(capacity_log2), C.byref(self._h))
        if rc:
            self._h = None
            raise ScopaError(rc, "scopa_full_mccfr_create", self._L.scopa_last_error(ctx._h).decode())
        self.capacity_log2 = int(capacity_log2)
        self.root = np.zeros(1, FULL_STATE_DTYPE)
        self._L.scopa_full_mccfr_root(self._h, _ptr(self.root), None, None)
        ctx._children.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_h", None):
            self._L.scopa_full_mccfr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, where):
        if rc:
            raise ScopaError(rc, where, self._L.scopa_last_error(self._ctx._h).decode())

    def cut(self, cut):
        self._ck(self._L.scopa_full_mccfr_cut(self._h, int(cut)), "scopa_full_mccfr_cut")

    def reset(self):
        self._ck(self._L.scopa_full_mccfr_reset(self._h), "scopa_full_mccfr_reset")

    def traverse(self, traverser, iteration, b0, nb):
        self._ck(self._L.scopa_full_mccfr_traverse(self._h, int(traverser), int(iteration), int(b0), int(nb)), "scopa_full_mccfr_traverse")

    def apply(self):
        self._ck(self._L.scopa_full_mccfr_apply(self._h), "scopa_full_mccfr_apply")

    def iterate(self, batch, n_iters=1):
        self._ck(self._L.scopa_full_mccfr_iterate(self._h, int(batch), int(n_iters)), "scopa_full_mccfr_iterate")

    def counters(self):
        """-> dict(choice_visits, terminal_visits, rows, dropped, iterations): exact integers"""
        c = [C.c_uint64() for _ in range(4)]
        it = C.c_uint32()
        self._ck(self._L.scopa_full_mccfr_counters(self._h, *[C.byref(x) for x in c], C.byref(it)), "scopa_full_mccfr_counters")
        return dict(choice_visits=c[0].value, terminal_visits=c[1].value, rows=c[2].value, dropped=c[3].value, iterations=it.value)

    def _rows(self, fn, name, third, fourth_dtype):
        n = C.c_int64(0)
        self._ck(fn(self._h, C.byref(n), None, None, None, None), name)
        m = max(n.value, 1)
        keys, a, b, x = np.zeros(m, np.uint64), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m, fourth_dtype)
        n = C.c_int64(m)
        args = (_ptr(keys), _ptr(x), _ptr(a), _ptr(b)) if third else (_ptr(keys), _ptr(a), _ptr(b), _ptr(x))
        self._ck(fn(self._h, C.byref(n), *args), name)
        order = np.argsort(keys[:n.value], kind="stable")
        return keys[:n.value][order], x[:n.value][order], a[:n.value][order], b[:n.value][order]

    def tables_get(self):
        """-> keys [n] uint64 ascending, n_act [n], regret [n][3], strategy [n][3]"""
        return self._rows(self._L.scopa_full_mccfr_tables_get, "scopa_full_mccfr_tables_get", True, np.int32)

    def delta_get(self):
        """-> keys [n] uint64 ascending, counts [n] uint32, d_regret [n][3], d_strategy [n][3]: what the traversals since the last apply added"""
        return self._rows(self._L.scopa_full_mccfr_delta_get, "scopa_full_mccfr_delta_get", False, np.uint32)

    def tables_set(self, keys, n_act, regret, strategy):
        keys = np.ascontiguousarray(keys, np.uint64)
        n_act = np.ascontiguousarray(n_act, np.int32)
        regret, strategy = np.ascontiguousarray(regret, np.float64).reshape(-1, 3), np.ascontiguousarray(strategy, np.float64).reshape(-1, 3)
        assert n_act.shape == keys.shape and regret.shape == strategy.shape == (keys.size, 3)
        self._ck(self._L.scopa_full_mccfr_tables_set(self._h, keys.size, _ptr(keys), _ptr(n_act), _ptr(regret), _ptr(strategy)), "scopa_full_mccfr_tables_set")

    def match(self, n_episodes, stream_id=0, per_episode=False):
        """-> sums [6] int64 (agent's rewards x2 in seat 0 / seat 1, their squares in seat 0 / seat 1, agent's scopas, opponent's scopas)
        and, with per_episode, the agent's reward x2 of every episode (int8)"""
        sums = np.zeros(6, np.int64)
        r2 = np.zeros(max(int(n_episodes), 1), np.int8) if per_episode else None
        self._ck(self._L.scopa_full_mccfr_match(self._h, int(n_episodes), int(stream_id), _ptr(sums), _ptr(r2)), "scopa_full_mccfr_match")
        return (sums, r2[:int(n_episodes)]) if per_episode else sums

    def exploitability(self, root=None, which=0):
        """Exact sweeps of the sub-game below `root` (a FULL_STATE_DTYPE record at a round boundary of this deck with at most 4 rounds to go; None =
        the handle's root) for the average policy (which = 0) or the current regret-matching sigma (which = 1)
        -> dict(exploitability=(br0 + br1) / 2, br0, br1, value).  br_p is the exact value, for player p, of a pure response built level by level;
        the infoset key has imperfect recall across rounds, so it is THE best response with one round to go and A response otherwise:
        `exploitability` is then a lower bound on the true one (include/scopa.h)."""
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        out = np.zeros(4, np.float64)
        self._ck(self._L.scopa_full_mccfr_exploitability(self._h, _ptr(root), int(which), _ptr(out)), "scopa_full_mccfr_exploitability")
        return dict(exploitability=float(out[0]), br0=float(out[1]), br1=float(out[2]), value=float(out[3]))

    def response_get(self, player):
        """-> keys [n] uint64 ascending, n_act [n] int32, action [n] int32 (the chosen slot), q [n][3]: the response of `player` from the last
        exploitability call"""
        n = C.c_int64(0)
        self._ck(self._L.scopa_full_mccfr_response_get(self._h, int(player), C.byref(n), None, None, None, None), "scopa_full_mccfr_response_get")
        m = max(n.value, 1)
        keys, n_act, action, q = np.zeros(m, np.uint64), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3))
        n = C.c_int64(m)
        self._ck(self._L.scopa_full_mccfr_response_get(self._h, int(player), C.byref(n), _ptr(keys), _ptr(n_act), _ptr(action), _ptr(q)), "scopa_full_mccfr_response_get")
        return keys[:n.value], n_act[:n.value], action[:n.value], q[:n.value]


def full_infoset_key_wide(state, player):
    """scopa_full_infoset_key_wide of a FULL_STATE_DTYPE record (or a FullState) -> (A, B): the deck-free key; host code, no GPU"""
    s = state.s if isinstance(state, FullState) else np.ascontiguousarray(state, FULL_STATE_DTYPE).reshape(1)
    key2 = (C.c_uint64 * 2)()
    rc = lib().scopa_full_infoset_key_wide(_ptr(s), int(player), C.byref(key2))
    if rc:
        raise ScopaError(rc, "scopa_full_infoset_key_wide")
    return int(key2[0]), int(key2[1])


def full_wide_key_fields(A, B):
    """a pair of scopa_full_infoset_key_wide -> dict(player, round, hand (cards in ascending id = action slots), table (cards, ascending id), ncap
    [player 0, player 1], scopas): everything scopa_full_state_infoset_string says, from the key alone"""
    A, B = int(A), int(B)
    player, rnd = (A >> 62) & 1, (A >> 59) & 7
    hand = [c for c in range(40) if (B >> c) & 1]
    table = [c for c in range(40) if (A >> (16 + c)) & 1]
    own = (A >> 10) & 63
    other = 4 + 6 * (rnd + 1) - len(table) - 2 * len(hand) + player - own       # the opponent holds as many cards (player 0 to move) or one fewer
    return dict(player=player, round=rnd, hand=hand, table=table, ncap=[other, own] if player else [own, other], scopas=[(A >> 5) & 31, A & 31])


def full_chance_sdcfr_features(keys2):
    """scopa_full_chance_sdcfr_features: the 96 advantage-net features of key pairs [n][2] -> float32 [n][96]; host code, no GPU"""
    keys2 = np.ascontiguousarray(keys2, np.uint64).reshape(-1, 2)
    feat = np.zeros((keys2.shape[0], 96), np.float32)
    rc = lib().scopa_full_chance_sdcfr_features(_ptr(keys2), keys2.shape[0], _ptr(feat))
    if rc:
        raise ScopaError(rc, "scopa_full_chance_sdcfr_features")
    return feat


def full_wide_key_to_string(A, B):
    """information_state_string (openspiel_full_scopa.py:79-94) of the decision node a key pair stands for, on whatever deck"""
    f = full_wide_key_fields(A, B)
    name = lambda cards: "-".join(f"{c % 10 + 1}{_FULL_SUITS[c // 10][0]}" for c in sorted(cards, key=lambda c: (c % 10 + 1, _FULL_SUITS[c // 10])))
    return (f"P{f['player']}:R{f['round']}:H[{name(f['hand'])}]:T[{name(f['table'])}]:C[{f['ncap'][0]},{f['ncap'][1]}]"
            f":S[{f['scopas'][0]},{f['scopas'][1]}]")


class FullSdcfrSnapshots(C.Structure):
    """scopa_full_sdcfr_snapshots of include/scopa.h"""
    _fields_ = [("n_snap", C.c_int32), ("max_size", C.c_int32)] + [(k, C.c_void_p) for k in ("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3", "h_slots", "d_coef")]


def _snapshot_sets(sets):
    """snapshot sets [(slots, six device pointers, max_size, coefficient pointer), ...] as an array of scopa_full_sdcfr_snapshots, and the slot arrays
    it points into (to keep alive over the call)"""
    sets = list(sets)
    arr, keep = (FullSdcfrSnapshots * len(sets))(), []
    for q, (slots, ptrs, max_size, coef_ptr) in enumerate(sets):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        keep.append(slots)
        arr[q].n_snap, arr[q].max_size = slots.size, int(max_size)
        for name, ptr in zip(("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3"), ptrs):
            setattr(arr[q], name, ptr or None)
        arr[q].h_slots, arr[q].d_coef = (slots.ctypes.data if slots.size else None), (coef_ptr or None)
    return arr, keep


class FullChanceMCCFR:
    """One scopa_full_chance: FullScopa over a set of decks below a common root, rows by the deck-free key pair (include/scopa.h)."""

    def __init__(self, ctx, decks, root=None, capacity_log2=22):
        import weakref
        self._h, self._ctx, self._L = C.c_void_p(), ctx, lib()
        self.decks = np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        rc = self._L.scopa_full_chance_create(ctx._h, _ptr(self.decks), self.decks.shape[0], _ptr(root), int(capacity_log2), C.byref(self._h))
        if rc:
            self._h = None
            raise ScopaError(rc, "scopa_full_chance_create", self._L.scopa_last_error(ctx._h).decode())
        self.capacity_log2, self.n_decks = int(capacity_log2), self.decks.shape[0]
        self.root = np.zeros(1, FULL_STATE_DTYPE)
        self._L.scopa_full_chance_root(self._h, _ptr(self.root), None, None, None)
        ctx._children.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_h", None):
            self._L.scopa_full_chance_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, where):
        if rc:
            raise ScopaError(rc, where, self._L.scopa_last_error(self._ctx._h).decode())

    def cut(self, cut):
        self._ck(self._L.scopa_full_chance_cut(self._h, int(cut)), "scopa_full_chance_cut")

    def reset(self):
        self._ck(self._L.scopa_full_chance_reset(self._h), "scopa_full_chance_reset")

    def traverse(self, traverser, iteration, b0, nb, decks=None):
        """nb traversals on each deck of `decks` (indices into the handle's decks; None = all)"""
        lst = None if decks is None else np.ascontiguousarray(decks, np.int32).reshape(-1)
        self._ck(self._L.scopa_full_chance_traverse(self._h, int(traverser), int(iteration), int(b0), int(nb), _ptr(lst), 0 if lst is None else lst.size),
                 "scopa_full_chance_traverse")

    def apply(self):
        self._ck(self._L.scopa_full_chance_apply(self._h), "scopa_full_chance_apply")

    def iterate(self, batch, n_iters=1, lists=None):
        """lists: [n_iters][m] deck indices, one list per iteration; None = every deck in every iteration"""
        if lists is not None:
            lists = np.ascontiguousarray(lists, np.int32)
            if lists.ndim != 2 or lists.shape[0] != int(n_iters):
                raise ValueError("lists must be [n_iters][m]")
        self._ck(self._L.scopa_full_chance_iterate(self._h, int(batch), int(n_iters), _ptr(lists), 0 if lists is None else lists.shape[1]), "scopa_full_chance_iterate")

    def counters(self):
        """-> dict(choice_visits, terminal_visits, rows, dropped, iterations): exact integers"""
        c = [C.c_uint64() for _ in range(4)]
        it = C.c_uint32()
        self._ck(self._L.scopa_full_chance_counters(self._h, *[C.byref(x) for x in c], C.byref(it)), "scopa_full_chance_counters")
        return dict(choice_visits=c[0].value, terminal_visits=c[1].value, rows=c[2].value, dropped=c[3].value, iterations=it.value)

    def _rows(self, fn, name, third, fourth_dtype):
        n = C.c_int64(0)
        self._ck(fn(self._h, C.byref(n), None, None, None, None), name)
        m = max(n.value, 1)
        keys, a, b, x = np.zeros((m, 2), np.uint64), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m, fourth_dtype)
        n = C.c_int64(m)
        args = (_ptr(keys), _ptr(x), _ptr(a), _ptr(b)) if third else (_ptr(keys), _ptr(a), _ptr(b), _ptr(x))
        self._ck(fn(self._h, C.byref(n), *args), name)
        order = np.lexsort((keys[:n.value, 1], keys[:n.value, 0]))
        return keys[:n.value][order], x[:n.value][order], a[:n.value][order], b[:n.value][order]

    def tables_get(self):
        """-> keys [n][2] uint64 sorted by (A, B), n_act [n], regret [n][3], strategy [n][3]"""
        return self._rows(self._L.scopa_full_chance_tables_get, "scopa_full_chance_tables_get", True, np.int32)

    def delta_get(self):
        """-> keys [n][2] uint64 sorted by (A, B), counts [n] uint32, d_regret [n][3], d_strategy [n][3]: what the traversals since the last apply added"""
        return self._rows(self._L.scopa_full_chance_delta_get, "scopa_full_chance_delta_get", False, np.uint32)

    def tables_set(self, keys, n_act, regret, strategy):
        keys = np.ascontiguousarray(keys, np.uint64).reshape(-1, 2)
        n_act = np.ascontiguousarray(n_act, np.int32)
        regret, strategy = np.ascontiguousarray(regret, np.float64).reshape(-1, 3), np.ascontiguousarray(strategy, np.float64).reshape(-1, 3)
        assert n_act.shape == (keys.shape[0],) and regret.shape == strategy.shape == (keys.shape[0], 3)
        self._ck(self._L.scopa_full_chance_tables_set(self._h, keys.shape[0], _ptr(keys), _ptr(n_act), _ptr(regret), _ptr(strategy)), "scopa_full_chance_tables_set")

    def match(self, n_episodes, stream_id=0, decks=None, per_episode=False):
        """-> sums [6] int64 as FullMCCFR.match and, with per_episode, the agent's reward x2 of every episode (int8); decks: [k][40] held-out decks
        that fit the handle's root, None = the handle's own"""
        sums = np.zeros(6, np.int64)
        r2 = np.zeros(max(int(n_episodes), 1), np.int8) if per_episode else None
        held = None if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        self._ck(self._L.scopa_full_chance_match(self._h, int(n_episodes), int(stream_id), _ptr(held), 0 if held is None else held.shape[0], _ptr(sums), _ptr(r2)),
                 "scopa_full_chance_match")
        return (sums, r2[:int(n_episodes)]) if per_episode else sums

    def exploitability(self, root=None, which=0, decks=None):
        """Exact sweeps of the sub-games below `root` (a FULL_STATE_DTYPE record at a round boundary, its hands ignored; None = the handle's root) on
        `decks` ([k][40] decks that fit that root, a deck listed twice counting twice; None = the handle's), the deal a uniform chance move, for the
        average policy (which = 0) or the current regret-matching sigma (which = 1) -> dict(exploitability=(br0 + br1) / 2, br0, br1, value).
        At most 4 rounds to go and k * 36^R <= 1 << 22.  br_p is the exact value, for player p, of a pure response that plays ONE action per key
        pair on every deck, built level by level; the key has imperfect recall across rounds, so with more than one round to go it is A response
        and `exploitability` a lower bound on the true one (include/scopa.h)."""
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        held = None if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        out = np.zeros(4, np.float64)
        self._ck(self._L.scopa_full_chance_exploitability(self._h, _ptr(root), _ptr(held), 0 if held is None else held.shape[0], int(which), _ptr(out)),
                 "scopa_full_chance_exploitability")
        return dict(exploitability=float(out[0]), br0=float(out[1]), br1=float(out[2]), value=float(out[3]))

    def cfr_iterate(self, n_iters, weights=None, alternating=True, root=None):
        """n_iters exact weighted CFR iterations on the sub-games below `root` (as for exploitability; None = the handle's root) on the handle's
        decks, the deal a uniform chance move; weights [n_iters][3] = (pos, neg, strat) per iteration, each in [0, 1] (None: all 1.0, vanilla CFR);
        alternating: player 0's rows, then a fresh sweep and player 1's, else both from one sweep -> the sweep values [n_iters][2] for player 0.
        At most 4 rounds to go and n_decks * 36^R <= 1 << 22; every pair of the forest is claimed in the store (ScopaError SCOPA_ENOMEM, with no
        row changed, where it is full along a probe).  The pair has imperfect recall across rounds: with more than one round to go CFR has no
        convergence proof here, and the figure to watch is exploitability()'s lower bound (include/scopa.h)."""
        n_iters = int(n_iters)
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.float64)
            if weights.shape != (n_iters, 3):
                raise ValueError("weights must be [n_iters][3]")
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        values = np.zeros((max(n_iters, 0), 2), np.float64)
        self._ck(self._L.scopa_full_chance_cfr_iterate(self._h, _ptr(root), n_iters, _ptr(weights), int(alternating), _ptr(values)), "scopa_full_chance_cfr_iterate")
        return values

    @staticmethod
    def cross_play(handles, root=None, which=0, decks=None):
        """The exact cross-play of K stores (scopa_full_chance_cross_play) -> float64 [K][K][4]: out[a][b] = (expected reward of player 0, expected
        square of it, expected scopas of player 0, of player 1) for handles[a] as player 0 against handles[b] as player 1 on the sub-games below
        `root` (None = handles[0]'s root) on `decks` ([k][40]; None = handles[0]'s), the deal a uniform chance move, for the average policies
        (which = 0) or the current regret-matching strategies (which = 1).  A handle may be listed more than once; all must be of one context;
        handles[0] owns the scratch.  K <= 16, at most 4 rounds to go, k * 36^R <= 1 << 22 and K * k * 36^R <= 1 << 24."""
        handles = list(handles)
        if not handles or any(getattr(h, "_h", None) is None for h in handles):
            raise ValueError("cross_play: needs at least one open FullChanceMCCFR handle")
        first = handles[0]
        hs = (C.c_void_p * len(handles))(*[h._h for h in handles])
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        held = None if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        out = np.zeros((len(handles), len(handles), 4), np.float64)
        first._ck(first._L.scopa_full_chance_cross_play(hs, len(handles), _ptr(root), _ptr(held), 0 if held is None else held.shape[0], int(which), _ptr(out)),
                  "scopa_full_chance_cross_play")
        return out

    def pair_match(self, other, n_episodes, stream_id=0, decks=None, per_episode=False):
        """-> sums [6] int64 as match and, with per_episode, this store's reward x2 of every episode (int8): the seat-swapped match from this handle's
        root of this store's average policy against `other`'s (scopa_full_chance_pair_match); decks as for match"""
        sums = np.zeros(6, np.int64)
        r2 = np.zeros(max(int(n_episodes), 1), np.int8) if per_episode else None
        held = None if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        self._ck(self._L.scopa_full_chance_pair_match(self._h, other._h, int(n_episodes), int(stream_id), _ptr(held), 0 if held is None else held.shape[0],
                                                      _ptr(sums), _ptr(r2)), "scopa_full_chance_pair_match")
        return (sums, r2[:int(n_episodes)]) if per_episode else sums

    # ---- sampled best response (scopa_full_chance_respond_*, _harden) ---------------------------------------------------------------------------------
    def respond_traverse(self, opp, which, responder, iteration, b0, nb, decks=None):
        """traverse with `responder` as the traverser and the other player a FIXED policy: `opp`'s store (another FullChanceMCCFR of this context; None =
        uniform play), its average policy (which = 0) or its current regret-matching sigma (which = 1).  Only the responder's rows of THIS store are
        claimed and added into; `opp` is read and left alone"""
        lst = None if decks is None else np.ascontiguousarray(decks, np.int32).reshape(-1)
        self._ck(self._L.scopa_full_chance_respond_traverse(self._h, None if opp is None else opp._h, int(which), int(responder), int(iteration), int(b0), int(nb),
                                                            _ptr(lst), 0 if lst is None else lst.size), "scopa_full_chance_respond_traverse")

    def respond_iterate(self, opp, which, batch, n_iters=1, lists=None):
        """n_iters iterations of respond_traverse(0), apply, respond_traverse(1), apply against `opp`; lists as for iterate"""
        if lists is not None:
            lists = np.ascontiguousarray(lists, np.int32)
            if lists.ndim != 2 or lists.shape[0] != int(n_iters):
                raise ValueError("lists must be [n_iters][m]")
        self._ck(self._L.scopa_full_chance_respond_iterate(self._h, None if opp is None else opp._h, int(which), int(batch), int(n_iters), _ptr(lists),
                                                           0 if lists is None else lists.shape[1]), "scopa_full_chance_respond_iterate")

    def harden(self):
        """every strategy row becomes the pure policy of its regret row (1.0 at the first maximal regret); regrets are untouched"""
        self._ck(self._L.scopa_full_chance_harden(self._h), "scopa_full_chance_harden")

    # ---- sampled best response to the Deep CFR nets (scopa_full_chance_respond_nets_*) ---------------------------------------------------------------
    def respond_nets_traverse(self, responder, opponent_set, iteration, b0, nb, decks=None, root=None):
        """respond_traverse at cut 0 with the nets' average policy as the fixed opponent, level by level, from any round-boundary root (`root`: a
        FULL_STATE_DTYPE record; None = the handle's): opponent_set is ONE snapshot set -- player 1 - responder's -- as (slots, six device pointers,
        max_size, coefficient pointer), the form sdcfr_match takes.  Only the responder's rows of THIS store are claimed and added into"""
        lst = None if decks is None else np.ascontiguousarray(decks, np.int32).reshape(-1)
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        arr, keep = _snapshot_sets([opponent_set])
        self._ck(self._L.scopa_full_chance_respond_nets_traverse(self._h, _ptr(root), int(responder), int(nb), _ptr(lst), 0 if lst is None else lst.size,
                                                                 C.cast(arr, C.c_void_p), int(iteration), int(b0)), "scopa_full_chance_respond_nets_traverse")
        del keep

    def respond_nets_iterate(self, sets, batch, n_iters=1, lists=None):
        """n_iters iterations of respond_nets_traverse(0), apply, respond_nets_traverse(1), apply from the handle's root against `sets`: two snapshot
        sets, player 0's and player 1's; lists as for iterate"""
        if lists is not None:
            lists = np.ascontiguousarray(lists, np.int32)
            if lists.ndim != 2 or lists.shape[0] != int(n_iters):
                raise ValueError("lists must be [n_iters][m]")
        sets = list(sets)
        if len(sets) != 2:
            raise ValueError("sets must be the two players' snapshot sets")
        arr, keep = _snapshot_sets(sets)
        self._ck(self._L.scopa_full_chance_respond_nets_iterate(self._h, C.cast(arr, C.c_void_p), int(batch), int(n_iters), _ptr(lists),
                                                                0 if lists is None else lists.shape[1]), "scopa_full_chance_respond_nets_iterate")
        del keep

    # ---- Deep CFR (scopa_full_chance_sdcfr_*) ---------------------------------------------------------------------------------------------------
    def sdcfr_traverse(self, traverser, batch, weight_ptrs, mem_feat_ptr, mem_regret_ptr, capacity, write_base, root_values_ptr, iteration, b0=0, decks=None,
                       root=None):
        """`batch` traversals of `traverser` on each deck of `decks` (indices into the handle's decks; None = all) into the memory ring at the device
        pointers given; weight_ptrs: six device pointers, each to the two players' tensors [2][...] in torch layout.  Queued on the context's stream."""
        vp = C.c_void_p
        lst = None if decks is None else np.ascontiguousarray(decks, np.int32).reshape(-1)
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        self._ck(self._L.scopa_full_chance_sdcfr_traverse(self._h, _ptr(root), int(traverser), int(batch), 0 if lst is None else lst.size, _ptr(lst),
                                                          *(vp(p) for p in weight_ptrs), vp(mem_feat_ptr), vp(mem_regret_ptr), int(capacity), int(write_base),
                                                          vp(root_values_ptr), int(iteration), int(b0)), "scopa_full_chance_sdcfr_traverse")

    def sdcfr_traverse_frontier(self, traverser, batch, weight_ptrs, mem_feat_ptr, mem_regret_ptr, capacity, write_base, root_values_ptr, iteration, b0=0, decks=None,
                                root=None):
        """sdcfr_traverse without a forest (scopa_full_chance_sdcfr_traverse_frontier): any round-boundary root, the deal included, any deck count;
        the same arguments, rows and ring positions; its draws are named by the path, so its samples differ from sdcfr_traverse's"""
        vp = C.c_void_p
        lst = None if decks is None else np.ascontiguousarray(decks, np.int32).reshape(-1)
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        self._ck(self._L.scopa_full_chance_sdcfr_traverse_frontier(self._h, _ptr(root), int(traverser), int(batch), 0 if lst is None else lst.size, _ptr(lst),
                                                                   *(vp(p) for p in weight_ptrs), vp(mem_feat_ptr), vp(mem_regret_ptr), int(capacity), int(write_base),
                                                                   vp(root_values_ptr), int(iteration), int(b0)), "scopa_full_chance_sdcfr_traverse_frontier")

    def sdcfr_match(self, n_episodes, agent, opponent=None, stream_id=0, decks=None, per_episode=False, trace=False):
        """The seat-swapped match from this handle's root of the nets' average policy (scopa_full_chance_sdcfr_match).  agent: two snapshot sets, player
        0's and player 1's, each (slots, param_ptrs, max_size, coef_ptr) as sdcfr_average_policy takes them; opponent: None (uniform play), a
        FullChanceMCCFR store of this context, or two more snapshot sets; decks as for match -> sums [6] int64 and, with per_episode, the agent's
        reward x2 of every episode (int8) and, with trace, the slot chosen at each of the game's 24 choice levels [n][24] int8 (-1 above the root)"""
        sets_of = _snapshot_sets
        n = int(n_episodes)
        a, keep_a = sets_of(agent)
        store, nets, keep_o = None, None, None
        if isinstance(opponent, FullChanceMCCFR):
            store = opponent._h
        elif opponent is not None:
            nets, keep_o = sets_of(opponent)
        sums = np.zeros(6, np.int64)
        r2 = np.zeros(max(n, 1), np.int8) if per_episode else None
        tr = np.zeros((max(n, 1), 24), np.int8) if trace else None
        held = None if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        self._ck(self._L.scopa_full_chance_sdcfr_match(self._h, n, int(stream_id), _ptr(held), 0 if held is None else held.shape[0], C.cast(a, C.c_void_p), store,
                                                       None if nets is None else C.cast(nets, C.c_void_p), _ptr(sums), _ptr(r2), _ptr(tr)), "scopa_full_chance_sdcfr_match")
        out = (sums,) + ((r2[:n],) if per_episode else ()) + ((tr[:n],) if trace else ())
        return out if len(out) > 1 else sums

    def debug_sdcfr_scratch(self, nbytes=0):
        """test hook: Context.full_chance_debug_sdcfr_scratch on this handle's context"""
        self._ctx.full_chance_debug_sdcfr_scratch(nbytes)

    def debug_sdcfr(self, launches=0):
        """benchmark hook: which launches sdcfr_traverse makes on this handle's context -- 0 both, 1 the policy launch alone, 2 the walk launch alone"""
        self._ck(self._L.scopa_full_chance_debug_sdcfr(self._ctx._h, int(launches)), "scopa_full_chance_debug_sdcfr")

    def sdcfr_visits(self):
        v = C.c_uint64()
        self._ck(self._L.scopa_full_chance_sdcfr_visits(self._h, C.byref(v)), "scopa_full_chance_sdcfr_visits")
        return v.value

    def sdcfr_policy_get(self):
        """-> (policy [T][3] float32, thresholds [T][2] uint64, keys [T][2] uint64) of the last sdcfr_traverse call's forest: every choice node,
        level-major and deck-major within a level"""
        n = C.c_int64(0)
        self._ck(self._L.scopa_full_chance_sdcfr_policy_get(self._h, C.byref(n), None, None, None), "scopa_full_chance_sdcfr_policy_get")
        T = n.value
        pol, thr, keys = np.zeros((T, 3), np.float32), np.zeros((T, 2), np.uint64), np.zeros((T, 2), np.uint64)
        self._ck(self._L.scopa_full_chance_sdcfr_policy_get(self._h, C.byref(n), _ptr(pol), _ptr(thr), _ptr(keys)), "scopa_full_chance_sdcfr_policy_get")
        return pol, thr, keys

    def sdcfr_average_policy(self, player, slots, param_ptrs, max_size, coef_ptr, decks=None, root=None):
        """The average of the snapshots `slots` (FIFO order; indices into six device tensors [max_size][...] at param_ptrs) with the float32
        coefficients at coef_ptr, at every choice node of `player` below `root` (None = the handle's) on `decks` ([k][40] decks that fit the root;
        None = the handle's) -> (keys [N][2] uint64, policy [N][3] float64), level-major and deck-major within a level.  Synchronous."""
        vp = C.c_void_p
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        root = None if root is None else np.ascontiguousarray(root, FULL_STATE_DTYPE).reshape(1)
        held = None if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        args = (self._h, _ptr(root), _ptr(held), 0 if held is None else held.shape[0], int(player), slots.size, *(vp(p) for p in param_ptrs), _ptr(slots) if slots.size else None,
                int(max_size), vp(coef_ptr))
        n = C.c_int64(0)
        self._ck(self._L.scopa_full_chance_sdcfr_average_policy(*args, C.byref(n), None, None), "scopa_full_chance_sdcfr_average_policy")
        keys, pol = np.zeros((n.value, 2), np.uint64), np.zeros((n.value, 3), np.float64)
        self._ck(self._L.scopa_full_chance_sdcfr_average_policy(*args, C.byref(n), _ptr(keys), _ptr(pol)), "scopa_full_chance_sdcfr_average_policy")
        return keys, pol

    def response_get(self, player):
        """-> keys [n][2] uint64 sorted by (A, B), n_act [n] int32, action [n] int32 (the chosen slot: the action-th held card in ascending id),
        q [n][3]: the response of `player` from the last exploitability call"""
        name = "scopa_full_chance_response_get"
        n = C.c_int64(0)
        self._ck(self._L.scopa_full_chance_response_get(self._h, int(player), C.byref(n), None, None, None, None), name)
        m = max(n.value, 1)
        keys, n_act, action, q = np.zeros((m, 2), np.uint64), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3))
        n = C.c_int64(m)
        self._ck(self._L.scopa_full_chance_response_get(self._h, int(player), C.byref(n), _ptr(keys), _ptr(n_act), _ptr(action), _ptr(q)), name)
        return keys[:n.value], n_act[:n.value], action[:n.value], q[:n.value]


def unpack_full_state(s):
    tab = [int((int(s["table"][i // 10]) >> (6 * (i % 10))) & 63) for i in range(int(s["nt"]))]
    hands = [[int((int(s["hand"][p]) >> (6 * i)) & 63) for i in range(int(s["nh"][p]))] for p in range(2)]
    caps = [[c for c in range(40) if (int(s["cap"][p]) >> c) & 1] for p in range(2)]
    last = int(s["last_capture"])
    return dict(hands=hands, table=tab, caps=caps, scopas=[int(s["scopas"][0]), int(s["scopas"][1])], round=int(s["round"]),
                step=int(s["step"]), deck_remaining=40 - int(s["deck_pos"]), last=-1 if last == 255 else last)


TEAM_STATE_DTYPE = np.dtype([("history", "<u8"), ("table", "<u4"), ("hand", "<u2", (4,)), ("cap", "<u2", (4,)), ("nh", "u1", (4,)),
                             ("scopas", "u1", (4,)), ("nt", "u1"), ("step", "u1"), ("last_capture_team", "u1"), ("flags", "u1")])
assert TEAM_STATE_DTYPE.itemsize == 40


class TeamState:
    """One packed Team MiniScopa TPI state driven through the host-side protocol (scopa_team_state_*)."""

    def __init__(self, seed=42, perm=None):
        self.perm = np.ascontiguousarray(deal_py_seed(seed) if perm is None else perm, np.uint8)
        self.s = np.zeros(1, TEAM_STATE_DTYPE)
        rc = lib().scopa_team_state_init(_ptr(self.perm), _ptr(self.s))
        if rc:
            raise ScopaError(rc, "scopa_team_state_init")

    def copy(self):
        c = TeamState.__new__(TeamState)
        c.perm, c.s = self.perm, self.s.copy()
        return c

    def step(self, action):
        rc = lib().scopa_team_state_step(_ptr(self.s), int(action))
        if rc:
            raise ScopaError(rc, "scopa_team_state_step")

    def legal(self):
        out, n = (C.c_int32 * 4)(), C.c_int32()
        lib().scopa_team_state_legal(_ptr(self.s), C.byref(out), C.byref(n))
        return [out[i] for i in range(n.value)]

    def is_terminal(self):
        return bool(int(self.s[0]["flags"]) & 1)

    def seat(self):
        return int(self.s[0]["step"]) & 3

    def current_player(self):
        return -4 if self.is_terminal() else self.seat() >> 1

    def player_rewards(self):
        r = (C.c_int32 * 4)()
        lib().scopa_team_state_rewards_x2(_ptr(self.s), C.byref(r))
        return [r[i] / 2.0 for i in range(4)]

    def rewards(self):
        """per TEAM (TPIMiniScopaState.rewards, openspiel_team_mini_scopa.py:106-116)"""
        if not self.is_terminal():
            return [0, 0]
        r = self.player_rewards()
        return [(r[0] + r[1]) / 2, (r[2] + r[3]) / 2]

    def infoset_string(self, team):
        buf = C.create_string_buffer(256)
        lib().scopa_team_state_infoset_string(_ptr(self.s), int(team), buf, 256)
        return buf.value.decode()

    def history(self):
        h = int(self.s[0]["history"])
        return [(h >> (4 * i)) & 15 for i in range(int(self.s[0]["step"]))]

    def history_str(self):
        h = "-".join(map(str, self.history()))
        if self.is_terminal():
            return f"TERMINAL:{h}:" + ",".join(f"{r:.2f}" for r in self.rewards())
        return f"H:{h}:T{self.current_player()}"

    def snapshot(self):
        d = unpack_team_state(self.s[0])
        d.update(cur=self.current_player(), legal=self.legal(), info0=self.infoset_string(0), info1=self.infoset_string(1),
                 hist=self.history_str(), rewards=[float(r) for r in self.rewards()])
        return d


def unpack_team_state(s):
    hands = [[(int(s["hand"][p]) >> (4 * i)) & 15 for i in range(int(s["nh"][p]))] for p in range(4)]
    last = int(s["last_capture_team"])
    return dict(hands=hands, table=[(int(s["table"]) >> (4 * i)) & 15 for i in range(int(s["nt"]))],
                caps=[[c for c in range(16) if (int(s["cap"][p]) >> c) & 1] for p in range(4)], scopas=[int(x) for x in s["scopas"]],
                last=-1 if last == 255 else last, step=int(s["step"]), seat=int(s["step"]) & 3, term=bool(int(s["flags"]) & 1))


class MultiDeal:
    """n independent deals resident on one device, one workgroup per deal (scopa_multi_* in include/scopa.h)."""

    def __init__(self, ctx, n_deals):
        self.ctx, self.n = ctx, int(n_deals)
        self._L = lib()
        self._h = C.c_void_p()
        ctx._ck(self._L.scopa_multi_create(ctx._h, self.n, C.byref(self._h)), "scopa_multi_create")
        self.n_infosets = None
        import weakref
        ctx._children.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_h", None):
            self._L.scopa_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def deal_py_seeds(self, seeds):
        s = np.ascontiguousarray(seeds, np.int64)
        assert s.size == self.n
        self.ctx._ck(self._L.scopa_multi_deal_py_seeds(self._h, _ptr(s)), "scopa_multi_deal_py_seeds")

    def set_perms(self, perms):
        p = np.ascontiguousarray(perms, np.uint8)
        assert p.shape == (self.n, 16)
        self.ctx._ck(self._L.scopa_multi_set_perms(self._h, _ptr(p)), "scopa_multi_set_perms")

    def perms(self):
        p = np.zeros((self.n, 16), np.uint8)
        self.ctx._ck(self._L.scopa_multi_perms_get(self._h, _ptr(p)), "scopa_multi_perms_get")
        return p

    def build(self):
        ninf = np.zeros(self.n, np.int32)
        self.ctx._ck(self._L.scopa_multi_build(self._h, _ptr(ninf)), "scopa_multi_build")
        self.n_infosets = ninf
        return ninf

    def cfr_exact_iterate(self, n_iters):
        self.ctx._ck(self._L.scopa_multi_cfr_exact_iterate(self._h, int(n_iters)), "scopa_multi_cfr_exact_iterate")

    def cfr_exact_iterate_lanes(self, n_iters):
        self.ctx._ck(self._L.scopa_multi_cfr_exact_iterate_lanes(self._h, int(n_iters)), "scopa_multi_cfr_exact_iterate_lanes")

    def cfr_sync_iterate(self, n_iters):
        self.ctx._ck(self._L.scopa_multi_cfr_sync_iterate(self._h, int(n_iters)), "scopa_multi_cfr_sync_iterate")

    def cfr_sync_iterate_weighted(self, weights, alternating=False, active=None):
        """Context.cfr_sync_iterate_weighted on every deal; active: bool / uint8 [n] (None = all), a deal with 0 is left untouched"""
        w, n = _weights(weights)
        a = None if active is None else np.ascontiguousarray(np.asarray(active) != 0, np.uint8)
        assert a is None or a.shape == (self.n,)
        self.ctx._ck(self._L.scopa_multi_cfr_sync_iterate_weighted(self._h, n, _ptr(w), int(alternating), _ptr(a)), "scopa_multi_cfr_sync_iterate_weighted")

    def solve(self, variant, eps, max_iters, check_every=10, alternating=False, **params):
        """Run `variant` ("vanilla", "cfr+", "linear", "dcfr"; params: alpha, beta, gamma) on every deal from iteration 1 until the deal's exploitability
        is below eps or max_iters is reached: chunks of check_every weighted iterations, exploitability() after each, the deals below eps dropped
        from the active mask.  -> int64 [n]: iterations each deal ran (a multiple of check_every, or max_iters).  Host logic over the mask alone."""
        from .algorithms.cfr_variants import schedule
        used, active, t = np.zeros(self.n, np.int64), np.ones(self.n, bool), 0
        while t < max_iters and active.any():
            k = min(int(check_every), int(max_iters) - t)
            self.cfr_sync_iterate_weighted(schedule(variant, t, k, **params), alternating, active)
            t += k
            used[active] = t
            active &= ~(self.exploitability()[:, 0] < eps)
        return used

    def mccfr_iterate(self, batch, n_iters, seed=0x5C09A):
        self.ctx._ck(self._L.scopa_multi_mccfr_iterate(self._h, int(batch), int(n_iters), int(seed)), "scopa_multi_mccfr_iterate")

    def exploitability(self):
        out = np.zeros((self.n, 4))
        self.ctx._ck(self._L.scopa_multi_exploitability(self._h, _ptr(out)), "scopa_multi_exploitability")
        return out

    def tables_get(self, deal):
        I = int(self.n_infosets[deal])
        R, S, Lc, K = np.zeros((I, 4)), np.zeros((I, 4)), np.zeros((I, 4)), np.zeros(I, np.uint64)
        self.ctx._ck(self._L.scopa_multi_tables_get(self._h, int(deal), _ptr(R), _ptr(S), _ptr(Lc), _ptr(K)), "scopa_multi_tables_get")
        return R, S, Lc, K

    def tables_set(self, deal, regret=None, strategy=None, local=None):
        arrs = []
        for a in (regret, strategy, local):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64)
                assert a.shape == (int(self.n_infosets[deal]), 4)
            arrs.append(a)
        self.ctx._ck(self._L.scopa_multi_tables_set(self._h, int(deal), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2])), "scopa_multi_tables_set")

    def counters(self):
        a, b = C.c_uint64(), C.c_uint64()
        self.ctx._ck(self._L.scopa_multi_counters(self._h, C.byref(a), C.byref(b)), "scopa_multi_counters")
        return a.value, b.value


class TeamChanceGame:
    """Team MiniScopa over a set of deals with the deal as a uniform chance move (scopa_team_chance_* in include/scopa.h): a team's rows are shared
    across deals by key, tables are [G][4] over the distinct keys.  `perms`: uint8 [n][16].  Owns a Context unless one is passed as `device`."""

    def __init__(self, perms, device=0):
        import weakref
        self.perms = np.ascontiguousarray(perms, np.uint8).reshape(-1, 16)
        self.ctx = device if isinstance(device, Context) else Context(device)
        self._own_ctx = not isinstance(device, Context)
        self._L = lib()
        self._h = C.c_void_p()
        self.ctx._ck(self._L.scopa_team_chance_create(self.ctx._h, self.perms.shape[0], _ptr(self.perms), C.byref(self._h)), "scopa_team_chance_create")
        n, G, occ = C.c_int32(), C.c_int64(), C.c_int64()
        self.ctx._ck(self._L.scopa_team_chance_counts(self._h, C.byref(n), C.byref(G), C.byref(occ)), "scopa_team_chance_counts")
        self.n, self.G, self.n_occurrences = n.value, G.value, occ.value
        self.ctx._children.insert(0, weakref.ref(self))   # closed before its context

    def close(self):
        if getattr(self, "_h", None):
            self._L.scopa_team_chance_destroy(self._h)
            self._h = None
            if self._own_ctx:
                self.ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self):
        import torch
        return torch.device("cuda", self.ctx.device)

    def index(self):
        """-> (keys uint64 [G] ascending, map int32 [n][TEAM_N_CHOICE]: local row -> global id)"""
        keys, mp = np.zeros(self.G, np.uint64), np.zeros((self.n, TEAM_N_CHOICE), np.int32)
        self.ctx._ck(self._L.scopa_team_chance_index_get(self._h, _ptr(keys), _ptr(mp)), "scopa_team_chance_index_get")
        return keys, mp

    def tables_reset(self):
        self.ctx._ck(self._L.scopa_team_chance_tables_reset(self._h), "scopa_team_chance_tables_reset")

    def tables_get(self):
        R, S = np.zeros((self.G, 4)), np.zeros((self.G, 4))
        self.ctx._ck(self._L.scopa_team_chance_tables_get(self._h, _ptr(R), _ptr(S)), "scopa_team_chance_tables_get")
        return R, S

    def tables_set(self, regret=None, strategy=None):
        arrs = []
        for a in (regret, strategy):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64)
                assert a.shape == (self.G, 4)
            arrs.append(a)
        self.ctx._ck(self._L.scopa_team_chance_tables_set(self._h, _ptr(arrs[0]), _ptr(arrs[1])), "scopa_team_chance_tables_set")

    def sigma_get(self):
        """the current strategy rows [G][4]: regret matching of the regret table"""
        L = np.zeros((self.G, 4))
        self.ctx._ck(self._L.scopa_team_chance_sigma_get(self._h, _ptr(L)), "scopa_team_chance_sigma_get")
        return L

    def cfr_iterate(self, weights_or_count, root_values=False):
        """one iteration per row (pos, neg, strat) of the weights; an int n runs n iterations with all weights 1.  -> root values [n][2] if asked"""
        if isinstance(weights_or_count, (int, np.integer)):
            w, n = None, int(weights_or_count)
        else:
            w, n = _weights(weights_or_count)
        rv = np.zeros((max(n, 0), 2))
        self.ctx._ck(self._L.scopa_team_chance_cfr_iterate(self._h, n, _ptr(w), _ptr(rv) if root_values and n > 0 else None), "scopa_team_chance_cfr_iterate")
        return rv if root_values else None

    def cfr_iterate_sampled(self, deals, weights=None, alternating=True, root_values=False):
        """deal-sampled iterations: iteration t sweeps only the deals of row t of `deals` (int [n_iters][m], distinct ids in [0, n)) and reduces over
        the listed occurrences; every row of an updated team is discounted.  `weights` None (all ones) or [n_iters][3] rows (pos, neg, strat).
        deals=None: all n deals every iteration, `weights` an int count or the weight rows -- the way to simultaneous updates (alternating=False)
        without a list.  -> root values [n_iters][2] (the listed deals' mean per traverser's sweep) if asked"""
        d, w, m = None, None, 0
        if deals is None:
            if isinstance(weights, (int, np.integer)):
                n = int(weights)
            elif weights is None:
                raise ValueError("deals=None needs weights: an iteration count or [n_iters][3] rows")
            else:
                w, n = _weights(weights)
        else:
            d = np.ascontiguousarray(deals, np.int32)
            if d.ndim != 2:
                raise ValueError("deals must be an int array [n_iters][m]")
            n, m = d.shape
            if weights is not None:
                w, nw = _weights(weights)
                if nw != n:
                    raise ValueError("weights must hold one row per row of deals")
        rv = np.zeros((max(n, 0), 2))
        self.ctx._ck(self._L.scopa_team_chance_cfr_iterate_sampled(self._h, n, m, _ptr(d), _ptr(w), int(alternating), _ptr(rv) if root_values and n > 0 else None),
                     "scopa_team_chance_cfr_iterate_sampled")
        return rv if root_values else None

    def cfr_launch(self, traverser, part):
        """one launch of an unweighted traversal, for timing: part 0 = the subtrees, 1 = the tops, 2 = the reduce"""
        self.ctx._ck(self._L.scopa_team_chance_cfr_launch(self._h, int(traverser), int(part)), "scopa_team_chance_cfr_launch")

    # ---- external-sampling MCCFR on the shared rows (scopa_team_chance_mccfr.hip); the Philox seed is the context's: game.ctx.mccfr_seed(seed) ----
    def mccfr_traverse(self, iteration, deal, b0, nb):
        """traversals [b0, b0 + nb) of `iteration`, one per traverser each, on deal `deal` against the shared regrets as they are; writes only the delta buffer"""
        self.ctx._ck(self._L.scopa_team_chance_mccfr_traverse(self._h, int(iteration), int(deal), int(b0), int(nb)), "scopa_team_chance_mccfr_traverse")

    def mccfr_apply(self):
        self.ctx._ck(self._L.scopa_team_chance_mccfr_apply(self._h), "scopa_team_chance_mccfr_apply")

    def mccfr_walk(self, iteration, batch, deals=None):
        """the walk launch of one iteration alone, for timing: `deals` an int list of distinct ids, None = all n deals"""
        d = None if deals is None else np.ascontiguousarray(deals, np.int32).reshape(-1)
        self.ctx._ck(self._L.scopa_team_chance_mccfr_walk(self._h, int(iteration), int(batch), 0 if d is None else d.size, _ptr(d)), "scopa_team_chance_mccfr_walk")

    def mccfr_iterate(self, batch, n_iters=1, deals=None):
        """deal-sampled external-sampling MCCFR on the shared rows: every iteration walks `batch` traversal pairs in each deal of its list -- row t of
        `deals` (int [n_iters][m], distinct ids in [0, n)), or all n deals when `deals` is None -- in ONE launch, with global traversal ids
        deal * batch + i and the handle's iteration number, then applies; rows without a listed occurrence are not touched"""
        d, m = None, 0
        if deals is not None:
            d = np.ascontiguousarray(deals, np.int32)
            if d.ndim != 2 or d.shape[0] != int(n_iters):
                raise ValueError("deals must be an int array [n_iters][m]")
            m = d.shape[1]
        self.ctx._ck(self._L.scopa_team_chance_mccfr_iterate(self._h, int(n_iters), int(batch), m, _ptr(d)), "scopa_team_chance_mccfr_iterate")

    def mccfr_counters(self):
        """-> (decision visits, terminal visits, MCCFR iterations) of this handle's MCCFR walks"""
        a, b, it = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self.ctx._ck(self._L.scopa_team_chance_mccfr_counters(self._h, C.byref(a), C.byref(b), C.byref(it)), "scopa_team_chance_mccfr_counters")
        return a.value, b.value, it.value

    def mccfr_delta_get(self):
        """the delta buffer [G][5]: 4 regret increments + traverser-visit count of the walks since the last apply"""
        d = np.zeros((self.G, 5))
        self.ctx._ck(self._L.scopa_team_chance_mccfr_delta_get(self._h, _ptr(d)), "scopa_team_chance_mccfr_delta_get")
        return d

    def exploitability(self, policy=None, return_policy=False, return_br=False):
        """-> out4 = [(BR0 + BR1) / 2, BR0, BR1, value for team 0] of `policy` ([G][4] numpy; None = the average policy); then, if asked, the evaluated
        policy [G][4] and the two best-response tables [2][G][4] (numpy)"""
        import torch
        dev = self._dev()
        out = (C.c_double * 4)()
        p = None
        if policy is not None:
            p = torch.from_numpy(np.ascontiguousarray(policy, np.float64)).to(dev)
            assert p.shape == (self.G, 4)
        po = torch.zeros((self.G, 4), dtype=torch.float64, device=dev) if return_policy else None
        br = torch.zeros((2, self.G, 4), dtype=torch.float64, device=dev) if return_br else None
        torch.cuda.synchronize(dev)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self.ctx._ck(self._L.scopa_team_chance_exploitability(self._h, ptr(p), C.byref(out), ptr(po), ptr(br)), "scopa_team_chance_exploitability")
        res = [np.array(out[:])]
        if return_policy:
            res.append(po.cpu().numpy())
        if return_br:
            res.append(br.cpu().numpy())
        return res[0] if len(res) == 1 else tuple(res)

    def best_response(self, policy=None):
        """-> (out4, br0, br1): exploitability(policy)'s numbers and the two best responses across deals as complete [G][4] tables (numpy), fit to go
        into cross_play or match"""
        out4, br = self.exploitability(policy, return_br=True)
        return out4, br[0], br[1]

    def cross_play(self, n_pol, policies_ptr, out_ptr, per_deal_ptr=0):
        """device pointers: policies [n_pol][G][4] float64 -> out [n_pol][n_pol][4], out[a][b] = exact (reward of team 0, its square, scopas of team 0,
        scopas of team 1) of table a as team 0 against table b as team 1 averaged over the deals, and (per_deal_ptr, or 0) the per-deal values
        [n][n_pol][n_pol][4]; three launches on the context's stream, no synchronisation"""
        vp = lambda x: C.c_void_p(x) if x else None
        self.ctx._ck(self._L.scopa_team_chance_cross_play(self._h, int(n_pol), vp(policies_ptr), vp(per_deal_ptr), vp(out_ptr)), "scopa_team_chance_cross_play")

    def match(self, policy_a_ptr, policy_b_ptr, n, n_team0, stream_id, deal_ptr=0, leaf_ptr=0):
        """Context.team_match with the deal drawn per episode (device pointers to two [G][4] float64 tables; episodes i < n_team0 have a as team 0)
        -> int64 [2][5] per half, from a's side; optionally every episode's deal and depth-12 index into int32 device buffers"""
        vp = lambda x: C.c_void_p(x) if x else None
        st = np.zeros((2, 5), np.int64)
        self.ctx._ck(self._L.scopa_team_chance_match(self._h, vp(policy_a_ptr), vp(policy_b_ptr), int(n), int(n_team0), stream_id, vp(deal_ptr), vp(leaf_ptr), _ptr(st)),
                     "scopa_team_chance_match")
        return st

    def policy_for_deal(self, policy, deal, as_tensor=False):
        """a global policy [G][4] (numpy or a float64 device tensor) in deal `deal`'s local row order -> float64 [TEAM_N_CHOICE][4], through the device scatter"""
        import torch
        dev = self._dev()
        pg = policy if isinstance(policy, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(policy, np.float64)).to(dev)
        assert pg.shape == (self.G, 4) and pg.dtype == torch.float64 and pg.is_contiguous()
        pl = torch.zeros((TEAM_N_CHOICE, 4), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.ctx._ck(self._L.scopa_team_chance_policy_for_deal(self._h, C.c_void_p(pg.data_ptr()), int(deal), C.c_void_p(pl.data_ptr())), "scopa_team_chance_policy_for_deal")
        self.ctx.synchronize()
        return pl if as_tensor else pl.cpu().numpy()

    def sdcfr_traverse(self, traverser, batch, weights_ptr, mem_feat_ptr, mem_regret_ptr, mem_mask_ptr, capacity, write_base, root_values_ptr,
                       iteration, b0=0, deals=None):
        """`batch` Deep CFR traversals of team `traverser` in each deal of `deals` (int [m], distinct ids in [0, n); None = all n deals) under the
        packed nets at weights_ptr (net p = team p), in two launches on the context's stream (no wait): traversal i of the deal in slot s has global
        id b0 + deal * batch + i, writes ring rows from (write_base + TEAM_SDCFR_ROWS * (s * batch + i)) % capacity and its root value to
        root_values[s * batch + i].  mem_mask_ptr may be 0."""
        d, m = None, 0
        if deals is not None:
            d = np.ascontiguousarray(deals, np.int32).reshape(-1)
            m = d.size
        vp = lambda x: C.c_void_p(x) if x else None
        self.ctx._ck(self._L.scopa_team_chance_sdcfr_traverse(self._h, int(traverser), int(batch), m, _ptr(d), vp(weights_ptr), vp(mem_feat_ptr), vp(mem_regret_ptr),
                                                              vp(mem_mask_ptr), int(capacity), int(write_base), vp(root_values_ptr), int(iteration), int(b0)),
                     "scopa_team_chance_sdcfr_traverse")

    def sdcfr_visits(self):
        """non-terminal visits of the handle's traversal calls: TEAM_SDCFR_VISITS[traverser] per traversal, counted on the host"""
        v = C.c_uint64()
        self.ctx._ck(self._L.scopa_team_chance_sdcfr_visits(self._h, C.byref(v)), "scopa_team_chance_sdcfr_visits")
        return v.value

    def sdcfr_policy_get(self, slot=0):
        """-> (policy float32 [TEAM_N_CHOICE][4], thresholds uint64 [TEAM_N_CHOICE][3]) of slot `slot` of the last traversal call, for tests (synchronises)"""
        pol, thr = np.zeros((TEAM_N_CHOICE, 4), np.float32), np.zeros((TEAM_N_CHOICE, 3), np.uint64)
        self.ctx._ck(self._L.scopa_team_chance_sdcfr_policy_get(self._h, int(slot), _ptr(pol), _ptr(thr)), "scopa_team_chance_sdcfr_policy_get")
        return pol, thr

    def sdcfr_forced_get(self, slot=0):
        """-> float32 [2][TEAM_N_LEAVES]: the policy of the one legal card at the last call's traverser's two forced depths, by depth-12 node, for tests"""
        f = np.zeros((2, TEAM_N_LEAVES), np.float32)
        self.ctx._ck(self._L.scopa_team_chance_sdcfr_forced_get(self._h, int(slot), _ptr(f)), "scopa_team_chance_sdcfr_forced_get")
        return f

    def sdcfr_average_policy(self, team, n_snap, param_ptrs, max_size, slots_ptr, coef_ptr, policy_ptr):
        """the rows of `team`'s keys in the [G][4] float64 device table at policy_ptr: Context.sdcfr_average_policy's average of n_snap snapshots of a
        StrategyBuffer store, evaluated once per distinct key (no wait)"""
        vp = lambda x: C.c_void_p(x) if x else None
        self.ctx._ck(self._L.scopa_team_chance_sdcfr_average_policy(self._h, int(team), int(n_snap), *(vp(p) for p in param_ptrs), int(max_size), vp(slots_ptr),
                                                                    vp(coef_ptr), vp(policy_ptr)), "scopa_team_chance_sdcfr_average_policy")

    def debug_sdcfr(self, terms_bytes=0, walk_groups=0, launches=0):
        """test and benchmark hooks on the context: bytes the terms of sdcfr_average_policy may take (keys go through in chunks that stay below it), the
        workgroups a slot of sdcfr_traverse's walk launch may have, and which launches a traversal call makes (1 the policy launch alone, 2 the walk
        launch alone over the tables of the call before); 0 restores a default"""
        self.ctx._ck(self._L.scopa_team_chance_debug_sdcfr(self.ctx._h, int(terms_bytes), int(walk_groups), int(launches)), "scopa_team_chance_debug_sdcfr")


class ChanceGame:
    """The n deals of a built MultiDeal as ONE game with the deal as a uniform chance move (scopa_chance_* in include/scopa.h): infosets are shared
    across deals by key, tables are [G][4] over the distinct keys.  The MultiDeal is borrowed and must stay built as it is while this object lives."""

    def __init__(self, multi):
        self.multi, self.ctx = multi, multi.ctx
        self._L = lib()
        self._h = C.c_void_p()
        self.ctx._ck(self._L.scopa_chance_create(multi._h, C.byref(self._h)), "scopa_chance_create")
        n, G, occ = C.c_int32(), C.c_int64(), C.c_int64()
        self.ctx._ck(self._L.scopa_chance_counts(self._h, C.byref(n), C.byref(G), C.byref(occ)), "scopa_chance_counts")
        self.n, self.G, self.n_occurrences = n.value, G.value, occ.value
        import weakref
        self.ctx._children.insert(0, weakref.ref(self))   # closed before the MultiDeal it borrows

    def close(self):
        if getattr(self, "_h", None):
            self._L.scopa_chance_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def index(self):
        """-> (keys uint64 [G] ascending, map int32 [n][1653]: local id -> global id, -1 beyond the deal's infoset count)"""
        keys, mp = np.zeros(self.G, np.uint64), np.zeros((self.n, N_DECISION), np.int32)
        self.ctx._ck(self._L.scopa_chance_index_get(self._h, _ptr(keys), _ptr(mp)), "scopa_chance_index_get")
        return keys, mp

    def tables_reset(self):
        self.ctx._ck(self._L.scopa_chance_tables_reset(self._h), "scopa_chance_tables_reset")

    def tables_get(self):
        R, S = np.zeros((self.G, 4)), np.zeros((self.G, 4))
        self.ctx._ck(self._L.scopa_chance_tables_get(self._h, _ptr(R), _ptr(S)), "scopa_chance_tables_get")
        return R, S

    def tables_set(self, regret=None, strategy=None):
        arrs = []
        for a in (regret, strategy):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64)
                assert a.shape == (self.G, 4)
            arrs.append(a)
        self.ctx._ck(self._L.scopa_chance_tables_set(self._h, _ptr(arrs[0]), _ptr(arrs[1])), "scopa_chance_tables_set")

    def cfr_iterate_weighted(self, weights, alternating=False):
        """one iteration per row (pos, neg, strat) of `weights`; an int n runs n iterations with all weights 1"""
        if isinstance(weights, (int, np.integer)):
            w, n = None, int(weights)
        else:
            w, n = _weights(weights)
        self.ctx._ck(self._L.scopa_chance_cfr_iterate_weighted(self._h, n, _ptr(w), int(alternating)), "scopa_chance_cfr_iterate_weighted")

    def cfr_iterate_sampled(self, deals, weights=None, alternating=False):
        """chance-sampled iterations: iteration t sweeps only the deals of row t of `deals` (int [n_iters][m], distinct ids in [0, n)) and reduces
        over the sampled occurrences; `weights` None (all ones) or [n_iters][3] rows (pos, neg, strat)"""
        d = np.ascontiguousarray(deals, np.int32)
        if d.ndim != 2:
            raise ValueError("deals must be an int array [n_iters][m]")
        n, m = d.shape
        w = None
        if weights is not None:
            w, nw = _weights(weights)
            if nw != n:
                raise ValueError("weights must hold one row per row of deals")
        self.ctx._ck(self._L.scopa_chance_cfr_iterate_sampled(self._h, n, m, _ptr(d), _ptr(w), int(alternating)), "scopa_chance_cfr_iterate_sampled")

    def mccfr_iterate(self, batch, n_iters=1, seed=0, deals=None):
        """chance-sampled external-sampling MCCFR on the shared rows: every iteration walks `batch` traversal pairs in each deal of its list --
        row t of `deals` (int [n_iters][m], distinct ids in [0, n)), or all n deals when `deals` is None -- with global traversal ids
        deal * batch + i, the handle's iteration number and `seed`; regret matching only, rows without a listed occurrence are not touched"""
        d, m = None, 0
        if deals is not None:
            d = np.ascontiguousarray(deals, np.int32)
            if d.ndim != 2 or d.shape[0] != int(n_iters):
                raise ValueError("deals must be an int array [n_iters][m]")
            m = d.shape[1]
        self.ctx._ck(self._L.scopa_chance_mccfr_iterate(self._h, int(n_iters), int(batch), int(seed), m, _ptr(d)), "scopa_chance_mccfr_iterate")

    def mccfr_counters(self):
        """-> (decision visits, terminal visits, MCCFR iterations) of this handle's MCCFR walks"""
        a, b, it = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self.ctx._ck(self._L.scopa_chance_mccfr_counters(self._h, C.byref(a), C.byref(b), C.byref(it)), "scopa_chance_mccfr_counters")
        return a.value, b.value, it.value

    def exploitability(self, policy=None, return_policy=False):
        """-> out4 = [(BR0 + BR1) / 2, BR0, BR1, value] of `policy` ([G][4]; None = the average policy), and the evaluated policy if asked"""
        out = np.zeros(4)
        p = None if policy is None else np.ascontiguousarray(policy, np.float64)
        assert p is None or p.shape == (self.G, 4)
        po = np.zeros((self.G, 4)) if return_policy else None
        self.ctx._ck(self._L.scopa_chance_exploitability(self._h, _ptr(p), _ptr(out), _ptr(po)), "scopa_chance_exploitability")
        return (out, po) if return_policy else out

    def policy_for_deal(self, policy, deal):
        """a global policy [G][4] (numpy) in deal `deal`'s local order -> float64 [n_infosets(deal)][4], through the device scatter"""
        import torch
        I = int(self.multi.n_infosets[deal])
        dev = torch.device("cuda", self.ctx.device)
        pg = torch.from_numpy(np.ascontiguousarray(policy, np.float64)).to(dev)
        assert pg.shape == (self.G, 4)
        pl = torch.zeros((I, 4), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.ctx._ck(self._L.scopa_chance_policy_for_deal(self._h, C.c_void_p(pg.data_ptr()), int(deal), C.c_void_p(pl.data_ptr())), "scopa_chance_policy_for_deal")
        return pl.cpu().numpy()

    def cross_play(self, n_pol, policies_ptr, out_ptr, per_deal_ptr=0):
        """device pointers: policies [n_pol][G][4] float64 -> out [n_pol][n_pol][4], out[a][b] = exact (reward of seat 0, its square, scopas of seat 0,
        scopas of seat 1) of policy a in seat 0 against policy b in seat 1 averaged over the deals, and (per_deal_ptr, or 0) the per-deal values
        [n][n_pol][n_pol][4]; two launches on the context's stream, no synchronisation"""
        vp = lambda x: C.c_void_p(x) if x else None
        self.ctx._ck(self._L.scopa_chance_cross_play(self._h, int(n_pol), vp(policies_ptr), vp(per_deal_ptr), vp(out_ptr)), "scopa_chance_cross_play")

    def best_response(self, n_pol, policies_ptr, br_ptr, out4_ptr):
        """device pointers: policies [n_pol][G][4] -> out4 [n_pol][4] = (exploitability, BR0, BR1, value) as exploitability() gives them per policy, and
        (br_ptr, or 0) br [n_pol][2][G][4]: the best-response tables themselves; on the context's stream, no synchronisation"""
        vp = lambda x: C.c_void_p(x) if x else None
        self.ctx._ck(self._L.scopa_chance_best_response(self._h, int(n_pol), vp(policies_ptr), vp(br_ptr), vp(out4_ptr)), "scopa_chance_best_response")

    def debug_scratch_budget(self, nbytes):
        """test hook: the scratch budget best_response chunks its policies by (0 restores 1 GiB)"""
        self.ctx._ck(self._L.scopa_chance_debug_scratch_budget(self._h, int(nbytes)), "scopa_chance_debug_scratch_budget")

    def match(self, policy_a_ptr, policy_b_ptr, n, n_seat0, stream_id, deal_ptr=0, idx_ptr=0):
        """Context.eval_pair_match with the deal drawn per episode (device pointers to two [G][4] float64 tables; episodes i < n_seat0 have a in seat 0)
        -> int64 [2][5] per seat half, from a's point of view; optionally every episode's deal and terminal index into int32 device buffers"""
        vp = lambda x: C.c_void_p(x) if x else None
        st = np.zeros((2, 5), np.int64)
        self.ctx._ck(self._L.scopa_chance_match(self._h, vp(policy_a_ptr), vp(policy_b_ptr), int(n), int(n_seat0), stream_id, vp(deal_ptr), vp(idx_ptr), _ptr(st)),
                     "scopa_chance_match")
        return st

    def sdcfr_traverse(self, traverser, batch, weights_ptr, mem_feat_ptr, mem_regret_ptr, mem_mask_ptr, capacity, write_base, root_values_ptr,
                       iteration, b0=0, deals=None):
        """`batch` Deep CFR traversals in each deal of `deals` (int [m], distinct ids in [0, n); None = all n deals) under the packed nets at
        weights_ptr, in two launches on the context's stream (no wait): traversal i of the deal in slot s has global id b0 + deal * batch + i, writes
        ring rows from (write_base + 41 * (s * batch + i)) % capacity and its root value to root_values[s * batch + i].  mem_mask_ptr may be 0."""
        d, m = None, 0
        if deals is not None:
            d = np.ascontiguousarray(deals, np.int32).reshape(-1)
            m = d.size
        vp = lambda x: C.c_void_p(x) if x else None
        self.ctx._ck(self._L.scopa_chance_sdcfr_traverse(self._h, int(traverser), int(batch), m, _ptr(d), vp(weights_ptr), vp(mem_feat_ptr), vp(mem_regret_ptr),
                                                         vp(mem_mask_ptr), int(capacity), int(write_base), vp(root_values_ptr), int(iteration), int(b0)),
                     "scopa_chance_sdcfr_traverse")

    def sdcfr_visits(self):
        v = C.c_uint64()
        self.ctx._ck(self._L.scopa_chance_sdcfr_visits(self._h, C.byref(v)), "scopa_chance_sdcfr_visits")
        return v.value

    def sdcfr_average_policy(self, player, n_snap, param_ptrs, max_size, slots_ptr, coef_ptr, policy_ptr):
        """the rows of `player`'s keys in the [G][4] float64 device table at policy_ptr: Context.sdcfr_average_policy's average of n_snap snapshots of a
        StrategyBuffer store, evaluated once per distinct key (no wait)"""
        vp = lambda x: C.c_void_p(x) if x else None
        self.ctx._ck(self._L.scopa_chance_sdcfr_average_policy(self._h, int(player), int(n_snap), *(vp(p) for p in param_ptrs), int(max_size), vp(slots_ptr),
                                                               vp(coef_ptr), vp(policy_ptr)), "scopa_chance_sdcfr_average_policy")
