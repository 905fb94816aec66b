"""ctypes view of the C ABI in include/abft_hip.h (libabft_hip.so).

The library is the product: there is no Python or CPU implementation behind
these calls.  If the shared object is missing or a call fails, this module
raises -- it never falls back to anything.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ABFT_HIP_LIB") or os.path.join(_HERE, "libabft_hip.so")  # override: A/B builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "abft_hip.h")

OK = 0
ERR_RANGE = -4  # ABFT_ERR_RANGE
MODES = ("none", "constraints", "sed", "sec7", "sec8", "secded")
MODE_ID = {m: i for i, m in enumerate(MODES)}
MODE_ID["sec"] = MODE_ID["sec7"]  # BASELINE.json config 5 spells sec7 "sec"
FMT_CSR, FMT_COO = 0, 1
FLIP_ANY, FLIP_VALUE, FLIP_INDEX = 0, 1, 2
PART_ALL, PART_INTERIOR, PART_BOUNDARY = 0, 1, 2
K_SPMV, K_DOT, K_CALC_XR, K_CALC_P = 0, 1, 2, 3
EV_VEC_CORRECTED, EV_VEC_DOUBLE = 10, 11  # protected vectors: bit = word bit | operand << 8
FMT_VECTOR = 2
EV_STRUCT_CORRECTED, EV_STRUCT_DOUBLE = 12, 13  # protected row structure: bit = word bit | kind << 8, index = row or block
STRUCT_ROW, STRUCT_BLOCK = 0, 1  # the kind of a structure word
EV_TRAIL_CORRECTED, EV_TRAIL_DOUBLE = 14, 15  # protected scalar trail: index = ordinal, bit = slot bit | record << 8
TRAIL_START, TRAIL_PW, TRAIL_NEXT = 0, 1, 2  # the record of a trail event
EV_MATRIX_DIGEST = 16  # a stored array of the matrix lost its armed digest: index = the segment kind, fatal
MAX_RHS = 8  # block right-hand sides per call (include/abft_hip.h)

u32p = C.POINTER(C.c_uint32)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int)
vp = C.c_void_p
vpp = C.POINTER(C.c_void_p)


class AbftError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("abft_hip error %d: %s" % (code, msg))
        self.code = code


class Event(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32), ("bit", C.c_uint32), ("fmt", C.c_uint32)]

    def tup(self):
        return (self.kind, self.index, self.bit)


# name -> (restype, argtypes); every symbol include/abft_hip.h declares
SIGNATURES = {
    "abft_hip_last_error": (C.c_char_p, []),
    "abft_hip_device_count": (C.c_int, [i32p]),
    "abft_hip_init": (C.c_int, [C.c_int, vpp]),
    "abft_hip_shutdown": (C.c_int, [vp]),
    "abft_hip_set_stream": (C.c_int, [vp, vp]),
    "abft_hip_get_stream": (vp, [vp]),
    "abft_hip_synchronize": (C.c_int, [vp]),
    "abft_hip_synchronize_timeout": (C.c_int, [vp, C.c_double]),
    "abft_hip_matrix_create_csr": (C.c_int, [vp, C.c_int, u32p, u32p, f64p, C.c_int, C.c_int, vpp]),
    "abft_hip_matrix_create_coo": (C.c_int, [vp, C.c_int, u32p, u32p, f64p, C.c_int, C.c_int, vpp]),
    "abft_hip_matrix_create_shard": (C.c_int, [vp, C.c_int, C.c_int, u32p, u32p, f64p, C.c_int, C.c_int,
                                               C.c_int, C.c_uint32, vpp]),
    "abft_hip_matrix_create_shard_indexed": (C.c_int, [vp, C.c_int, C.c_int, u32p, u32p, f64p, C.c_int, C.c_int,
                                                       C.c_int, u32p, vpp]),
    "abft_hip_matrix_destroy": (C.c_int, [vp]),
    "abft_hip_matrix_info": (C.c_int, [vp, i32p, i32p]),
    "abft_hip_matrix_compact_stats": (C.c_int, [vp, u32p, u32p, u32p]),
    "abft_hip_matrix_packed_stats": (C.c_int, [vp, u32p, u32p, u32p]),
    "abft_hip_packed_stats": (C.c_int, [vp, u32p, u32p, u32p]),
    "abft_hip_matrix_read_element": (C.c_int, [vp, C.c_uint32, u32p]),
    "abft_hip_matrix_read_csr": (C.c_int, [vp, vp, vp, vp]),
    "abft_hip_matrix_read_coo": (C.c_int, [vp, vp]),
    "abft_hip_inject": (C.c_int, [vp, C.c_uint32, i32p, C.c_int]),
    "abft_hip_inject_rowptr": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
    "abft_hip_matrix_create_csr_protected": (C.c_int, [vp, C.c_int, u32p, u32p, f64p, C.c_int, C.c_int, vpp]),
    "abft_hip_matrix_structure_info": (C.c_int, [vp, i32p, u32p, u32p]),
    "abft_hip_matrix_read_structure": (C.c_int, [vp, vp, vp]),
    "abft_hip_matrix_write_structure": (C.c_int, [vp, vp, vp]),
    "abft_hip_inject_structure": (C.c_int, [vp, C.c_int, C.c_uint32, i32p, C.c_int]),
    "abft_hip_matrix_scrub_structure": (C.c_int, [vp, vp, u32p, u32p]),
    "abft_hip_vector_create": (C.c_int, [vp, C.c_int, vpp]),
    "abft_hip_vector_view": (C.c_int, [vp, C.c_int, C.c_int, vpp]),
    "abft_hip_vector_destroy": (C.c_int, [vp]),
    "abft_hip_vector_map": (C.c_int, [vp, C.POINTER(f64p)]),
    "abft_hip_vector_unmap": (C.c_int, [vp, f64p]),
    "abft_hip_vector_copy": (C.c_int, [vp, vp]),
    "abft_hip_vector_device_ptr": (vp, [vp]),
    "abft_hip_vector_length": (C.c_int, [vp]),
    "abft_hip_dot": (C.c_int, [vp, vp, vp, f64p]),
    "abft_hip_calc_xr": (C.c_int, [vp, vp, vp, vp, vp, C.c_double, f64p]),
    "abft_hip_calc_p": (C.c_int, [vp, vp, vp, C.c_double]),
    "abft_hip_spmv": (C.c_int, [vp, vp, vp, vp]),
    "abft_hip_matrix_create_csr_stream": (C.c_int, [vp, C.c_int, u32p, u32p, f64p, C.c_int, C.c_int, vpp]),
    "abft_hip_spmm": (C.c_int, [vp, vp, vp, vp, C.c_int]),
    "abft_hip_dot_block": (C.c_int, [vp, vp, vp, C.c_int, f64p]),
    "abft_hip_calc_xr_block": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, f64p, C.c_uint32, f64p]),
    "abft_hip_calc_p_block": (C.c_int, [vp, vp, vp, C.c_int, f64p, C.c_uint32]),
    "abft_hip_vector_flip": (C.c_int, [vp, C.c_int, i32p, C.c_int]),
    "abft_hip_vector_encode": (C.c_int, [vp, vp]),
    "abft_hip_vector_scrub": (C.c_int, [vp, vp, i32p, i32p]),
    "abft_hip_spmv_vecc": (C.c_int, [vp, vp, vp, vp]),
    "abft_hip_dot_vecc": (C.c_int, [vp, vp, vp, f64p]),
    "abft_hip_calc_xr_vecc": (C.c_int, [vp, vp, vp, vp, vp, C.c_double, f64p]),
    "abft_hip_calc_p_vecc": (C.c_int, [vp, vp, vp, C.c_double]),
    "abft_hip_calc_r_vecc": (C.c_int, [vp, vp, vp, C.c_double, f64p]),
    "abft_hip_calc_px_vecc": (C.c_int, [vp, vp, vp, vp, C.c_double, C.c_double]),
    "abft_hip_precond_start_vecc": (C.c_int, [vp, vp, vp, vp, f64p]),
    "abft_hip_calc_r_precond_vecc": (C.c_int, [vp, vp, vp, vp, C.c_double, f64p]),
    "abft_hip_calc_px_precond_vecc": (C.c_int, [vp, vp, vp, vp, vp, C.c_double, C.c_double]),
    "abft_hip_residual_gap": (C.c_int, [vp, vp, vp, vp, vp, vp, f64p]),
    "abft_hip_residual_restart": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f64p]),
    "abft_hip_residual_gap_block": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_uint32, f64p]),
    "abft_hip_residual_restart_block": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_uint32, f64p]),
    "abft_hip_copy_block": (C.c_int, [vp, vp, vp, C.c_int, C.c_uint32]),
    "abft_hip_matrix_diag_inverse": (C.c_int, [vp, vp, vp, u32p]),
    "abft_hip_precond_start": (C.c_int, [vp, vp, vp, vp, f64p]),
    "abft_hip_calc_xr_precond": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_double, f64p]),
    "abft_hip_calc_p_precond": (C.c_int, [vp, vp, vp, vp, C.c_double]),
    "abft_hip_precond_start_block": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_uint32, f64p]),
    "abft_hip_calc_xr_precond_block": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, f64p, C.c_uint32, f64p]),
    "abft_hip_calc_p_precond_block": (C.c_int, [vp, vp, vp, vp, C.c_int, f64p, C.c_uint32]),
    "abft_hip_spmm_dot": (C.c_int, [vp, vp, vp, vp, C.c_int, f64p]),
    "abft_hip_calc_r_block": (C.c_int, [vp, vp, vp, C.c_int, f64p, C.c_uint32, f64p]),
    "abft_hip_calc_px_block": (C.c_int, [vp, vp, vp, vp, C.c_int, f64p, f64p, C.c_uint32]),
    "abft_hip_calc_r_precond_block": (C.c_int, [vp, vp, vp, vp, C.c_int, f64p, C.c_uint32, f64p]),
    "abft_hip_calc_px_precond_block": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, f64p, f64p, C.c_uint32]),
    "abft_hip_spmm_dot_vecc": (C.c_int, [vp, vp, vp, vp, C.c_int, f64p]),
    "abft_hip_dot_block_vecc": (C.c_int, [vp, vp, vp, C.c_int, f64p]),
    "abft_hip_calc_r_block_vecc": (C.c_int, [vp, vp, vp, C.c_int, f64p, C.c_uint32, f64p]),
    "abft_hip_calc_px_block_vecc": (C.c_int, [vp, vp, vp, vp, C.c_int, f64p, f64p, C.c_uint32]),
    "abft_hip_dot_dev": (C.c_int, [vp, vp, vp, vp]),
    "abft_hip_calc_xr_dev": (C.c_int, [vp, vp, vp, vp, vp, C.c_double, vp]),
    "abft_hip_read_pair": (C.c_int, [vp, vp, f64p, f64p]),
    "abft_hip_spmv_dot_dev": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
    "abft_hip_matrix_set_interior": (C.c_int, [vp, C.c_int, C.c_int]),
    "abft_hip_spmv_part": (C.c_int, [vp, vp, vp, vp, C.c_int]),
    "abft_hip_spmv_dot_part_dev": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.c_int]),
    "abft_hip_calc_xr_ratio_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "abft_hip_calc_p_ratio_dev": (C.c_int, [vp, vp, vp, vp, vp]),
    "abft_hip_set_sharers": (C.c_int, [vp, C.c_int]),
    "abft_hip_speculation_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "abft_hip_cg_iteration_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "abft_hip_tail_stats": (C.c_int, [vp, i32p, i32p, i32p, C.POINTER(C.c_long)]),
    "abft_hip_x_in_spmv_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "abft_hip_lazy_x_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "abft_hip_ahead_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "abft_hip_cg_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_double]),
    "abft_hip_cg_vecc_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                                      C.c_double]),
    "abft_hip_pcg_vecc_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                                       C.c_double]),
    "abft_hip_pcg_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                                   C.c_double]),
    "abft_hip_cg_trail_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                                       C.c_double]),
    "abft_hip_pcg_trail_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                                        C.c_double]),
    "abft_hip_cg_vecc_trail_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                                            C.c_double]),
    "abft_hip_pcg_vecc_trail_iteration_until_dev": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                                             vp, C.c_double]),
    "abft_hip_trail_encode": (C.c_int, [f64p, C.c_int, C.c_int, f64p]),
    "abft_hip_trail_decode": (C.c_int, [f64p, C.c_int, f64p, i32p, i32p]),
    "abft_hip_trail_flip": (C.c_int, [vp, vp, C.c_int, i32p, C.c_int]),
    "abft_hip_trail_inject_at": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, i32p, C.c_int]),
    "abft_hip_cg_block_iteration_until_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_double]),
    "abft_hip_cg_block_vecc_iteration_until_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_double]),
    "abft_hip_block_loop_reserve": (C.c_int, [vp, vp, C.c_int]),
    "abft_hip_cg_block_trail_iteration_until_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp,
                                                              C.c_double]),
    "abft_hip_cg_block_vecc_trail_iteration_until_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp,
                                                                   C.c_double]),
    "abft_hip_block_trail_inject_at": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, i32p, C.c_int]),
    "abft_hip_residual_check_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_double]),
    "abft_hip_residual_check_reserve": (C.c_int, [vp]),
    "abft_hip_write_pair": (C.c_int, [vp, vp, C.c_double, C.c_double]),
    "abft_hip_peer_board_bytes": (C.c_size_t, []),
    "abft_hip_peer_board_attach": (C.c_int, [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_double]),
    "abft_hip_peer_board_detach": (C.c_int, [vp]),
    "abft_hip_allreduce_pair_peers": (C.c_int, [vp, vp]),
    "abft_hip_peer_board_failed": (C.c_int, [vp]),
    "abft_hip_peer_board_ipc_handle_bytes": (C.c_size_t, []),
    "abft_hip_peer_board_ipc_export": (C.c_int, [vp, vp]),
    "abft_hip_peer_board_ipc_attach": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_double]),
    "abft_hip_peer_board_device_alloc": (C.c_int, [vp, C.POINTER(vp)]),
    "abft_hip_peer_board_device_free": (C.c_int, [vp, vp]),
    "abft_hip_peer_board_attach_device": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_double]),
    "abft_hip_peer_board_fuse": (C.c_int, [vp, C.c_int]),
    "abft_hip_peer_exchange_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "abft_hip_peer_exchange_attach": (C.c_int, [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, vp,
                                                C.c_int, C.c_double]),
    "abft_hip_peer_exchange_detach": (C.c_int, [vp]),
    "abft_hip_peer_exchange": (C.c_int, [vp, vp]),
    "abft_hip_peer_exchange_begin": (C.c_int, [vp, vp, C.c_int]),
    "abft_hip_peer_exchange_finish": (C.c_int, [vp]),
    "abft_hip_peer_exchange_failed": (C.c_int, [vp]),
    "abft_hip_peer_exchange_ipc_export": (C.c_int, [vp, C.c_int, C.c_size_t, vp]),
    "abft_hip_peer_exchange_ipc_attach": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, vp, C.c_int,
                                                    C.c_double]),
    "abft_hip_peer_exchange_device_alloc": (C.c_int, [vp, C.c_int, C.c_size_t, C.POINTER(vp)]),
    "abft_hip_peer_exchange_device_free": (C.c_int, [vp, vp]),
    "abft_hip_peer_exchange_attach_device": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_size_t, vp, C.c_int, vp,
                                                       C.c_int, C.c_double]),
    "abft_hip_matrix_panels": (C.c_int, [vp, i32p, i32p]),
    "abft_hip_spmv_dot_range_dev": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int]),
    "abft_hip_graph_begin": (C.c_int, [vp]),
    "abft_hip_graph_end": (C.c_int, [vp, vpp]),
    "abft_hip_graph_launch": (C.c_int, [vp]),
    "abft_hip_graph_destroy": (C.c_int, [vp]),
    "abft_hip_segment_name": (C.c_char_p, [C.c_uint32]),
    "abft_hip_matrix_segments": (C.c_int, [vp, u32p, C.POINTER(C.c_uint64), C.c_int, i32p]),
    "abft_hip_matrix_digest": (C.c_int, [vp, vp, C.POINTER(C.c_uint64), C.c_int]),
    "abft_hip_matrix_digest_arm": (C.c_int, [vp, vp]),
    "abft_hip_matrix_verify": (C.c_int, [vp, vp, i32p, u32p, C.c_int]),
    "abft_hip_matrix_verify_dev": (C.c_int, [vp, vp]),
    "abft_hip_matrix_read_segment": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint64]),
    "abft_hip_matrix_flip_segment": (C.c_int, [vp, vp, C.c_uint32, C.c_uint64, i32p, C.c_int]),
    "abft_hip_drain_events": (C.c_int, [vp, C.POINTER(Event), C.c_int, i32p, i32p]),
    "abft_hip_event_capacity": (C.c_int, []),
    "abft_hip_pending_events": (C.c_int, [vp]),
    "abft_format_event": (C.c_int, [C.POINTER(Event), C.c_char_p, C.c_size_t]),
    "abft_event_is_fatal": (C.c_int, [C.c_uint32]),
    "abft_hip_profile_enable": (C.c_int, [vp, C.c_int]),
    "abft_hip_profile_stride": (C.c_int, [vp, C.c_int]),
    "abft_hip_profile_reset": (C.c_int, [vp]),
    "abft_hip_profile_read": (C.c_int, [vp, C.c_int, f64p, C.POINTER(C.c_long)]),
    "abft_hip_stream_probe": (C.c_int, [vp, C.c_size_t, C.c_int, f64p, f64p]),
}

_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so (same soname as /opt/rocm's); if libabft_hip.so pulled in
    ROCm's copy and torch later loaded its own, the second runtime to start finds
    no device.  When torch is installed, load ITS runtime first (without importing
    torch): libabft_hip.so then binds to it by soname, and so does torch whenever
    it is imported.  Plain C++ users of the library (cg-csr / cg-coo) never load
    torch and run on /opt/rocm's runtime.  ABFT_HIP_SYSTEM_RUNTIME=1 skips this."""
    if os.environ.get("ABFT_HIP_SYSTEM_RUNTIME") == "1":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        return
    rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)


def load():
    """Load libabft_hip.so (built by `make -C abft_sparse_cg_amd/csrc`).  Raises
    if it is missing: the HIP library is the only implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not found: build it with `make -C %s` (hipcc --offload-arch=gfx950); "
                              "there is no CPU fallback" % (LIB_PATH, os.path.join(_HERE, "csrc")))
        _share_torch_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc != OK:
        raise AbftError(rc, (load().abft_hip_last_error() or b"").decode(errors="replace"))


def is_fatal(kind):
    """same rule as abft_event_is_fatal"""
    return kind in (1, 4, EV_VEC_DOUBLE, EV_STRUCT_DOUBLE, EV_TRAIL_DOUBLE, EV_MATRIX_DIGEST) or 5 <= kind <= 9


# the segment kinds of the matrix digests (csrc/matrix_digest.h, ABFT_SEG_*), by name: asked of the library once
SEG_COUNT = 64  # room for every kind the list can hold
_seg_names = None


def segment_names():
    """-> the names of the segment kinds, kind k at index k ("none" at 0)"""
    global _seg_names
    if _seg_names is None:
        names, k = [], 0
        while True:
            s = load().abft_hip_segment_name(k)
            if s is None:
                break
            names.append(s.decode())
            k += 1
        _seg_names = names
    return _seg_names


def segment_name(kind):
    names = segment_names()
    return names[kind] if 0 <= kind < len(names) else "?"


def segment_kind(name):
    names = segment_names()
    if name not in names or name == "none":
        raise ValueError("unknown matrix segment %r (one of %s)" % (name, ", ".join(names[1:])))
    return names.index(name)


def format_event(kind, index, bit, fmt):
    buf = C.create_string_buffer(160)
    ev = Event(kind, index, bit, fmt)
    load().abft_format_event(C.byref(ev), buf, 160)
    return buf.value.decode()
