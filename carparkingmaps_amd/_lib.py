"""Loader of the product library carparkingmaps_amd/csrc/libcpm_hip.so (C ABI: include/cpm.h).

There is no CPU fallback: if the library is missing or no HIP device is usable, every
compute entry point raises.  The oracle under oracle/ is never imported from here.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("CPM_LIB_PATH") or os.path.join(CSRC, "libcpm_hip.so")  # override: diagnostic twin, tools only

# every symbol include/cpm.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "cpm_last_error", "cpm_version", "cpm_device_count", "cpm_device_info", "cpm_create", "cpm_destroy",
    "cpm_set_option", "cpm_set_stream", "cpm_sync", "cpm_set_p_drive", "cpm_set_p_dest", "cpm_set_datamatrix",
    "cpm_build_p_drive", "cpm_build_p_dest", "cpm_get_p_drive", "cpm_get_cdf_row", "cpm_init_states",
    "cpm_set_state", "cpm_get_state", "cpm_solve_ivp", "cpm_resample", "cpm_resample_dev",
    "cpm_solve_ivp_async", "cpm_synth_tables", "cpm_last_kernel_ms", "cpm_algorithmic_bytes_per_hour",
    "cpm_debug_categorical", "cpm_createdatamatrix_rows", "cpm_createdatamatrix_csv", "cpm_get_datamatrix",
    "cpm_set_distance_from_centroids", "cpm_get_distance", "cpm_parse_uber_csv", "cpm_set_distance", "cpm_get_info",
    "cpm_init_states_strided", "cpm_synth_tables_skewed", "cpm_synth_datamatrix", "cpm_refresh_tables",
    "cpm_debug_travel_draw", "cpm_debug_f64_kit",
]

# every symbol include/cpm_batch.h declares (checked by tests/test_batch_host.py); kept apart: SYMBOLS is cpm.h's list
BATCH_SYMBOLS = ["cpm_set_p_drive_batch", "cpm_build_p_drive_batch", "cpm_get_p_drive_batch", "cpm_resample_batch", "cpm_resample_batch_dev"]

# every symbol include/cpm_flows.h declares (checked by tests/test_flows.py); kept apart like the batch list
FLOWS_SYMBOLS = ["cpm_resample_flows", "cpm_resample_flows_dev"]

# every symbol include/cpm_flows_csr.h declares (checked by tests/test_flows_csr.py); a header and a list of its own, likewise
FLOWS_CSR_SYMBOLS = ["cpm_resample_flows_csr_dev", "cpm_resample_flows_csr", "cpm_get_flows_csr"]

# every symbol include/cpm_stays.h declares (checked by tests/test_stays.py); a header and a list of its own, likewise
STAYS_SYMBOLS = ["cpm_resample_stays", "cpm_resample_stays_dev"]

# every symbol include/cpm_paths.h declares (checked by tests/test_paths.py); a header and a list of its own, likewise
PATHS_SYMBOLS = ["cpm_resample_paths", "cpm_resample_paths_dev", "cpm_paths_expand_dev"]

# every symbol include/cpm_charge.h declares (checked by tests/test_charge.py); a header and a list of its own, likewise
CHARGE_SYMBOLS = ["cpm_resample_charge", "cpm_resample_charge_dev"]


class ChargeParamsC(C.Structure):
    """cpm_charge_params of include/cpm_charge.h"""
    _fields_ = [("capacity_wh", C.c_uint32), ("power_wh", C.c_uint32), ("initial_wh", C.c_uint32), ("wh_per_km", C.c_double),
                ("zone_power_wh", C.c_void_p), ("soc_in", C.c_void_p)]


# every symbol include/cpm_objectives.h declares (checked by tests/test_objectives.py); a header and a list of its own, likewise
OBJECTIVES_SYMBOLS = ["cpm_set_measured", "cpm_objectives_dev"]

# every symbol include/cpm_expected.h declares (checked by tests/test_expected.py); a header and a list of its own, likewise
EXPECTED_SYMBOLS = ["cpm_expected_dev", "cpm_expected_batch_dev", "cpm_expected", "cpm_expected_batch"]
CPM_EXPECT_IVP = 1  # flags of the expected calls: start the day from pi0 carried through hours 0 .. T-2
CPM_FIT_DEST = 0x100  # flag of the expected_fit calls: also dF/de_dest along the installed tangent
CPM_FIT_WORDS = 16    # words of an expected_fit record in front of the traffic activity

# every symbol include/cpm_expected_travel.h declares (checked by tests/test_expected_travel.py); a header and a list of its own, likewise
EXPECTED_TRAVEL_SYMBOLS = ["cpm_expected_trip_dev", "cpm_expected_trip", "cpm_expected_travel_dev", "cpm_expected_travel",
                           "cpm_expected_travel_batch", "cpm_expected_trip_builds"]

# every symbol include/cpm_expected_grad.h declares (checked by tests/test_expected_grad.py); a header and a list of its own, likewise
EXPECTED_GRAD_SYMBOLS = ["cpm_expected_grad_dev", "cpm_expected_grad"]

# every symbol include/cpm_expected_grad_dest.h declares (checked by tests/test_expected_grad_dest.py); a header and a list of its own, likewise
EXPECTED_GRAD_DEST_SYMBOLS = ["cpm_set_p_dest_tangent", "cpm_build_p_dest_tangent", "cpm_get_p_dest_tangent", "cpm_expected_grad_dest_dev",
                              "cpm_expected_grad_dest", "cpm_expected_trip_tangent_dev", "cpm_expected_trip_tangent"]

# every symbol include/cpm_expected_grad_batch.h declares (checked by tests/test_expected_grad_batch.py); a header and a list of its own, likewise
EXPECTED_GRAD_BATCH_SYMBOLS = ["cpm_expected_grad_batch_dev", "cpm_expected_grad_batch", "cpm_expected_grad_dest_batch_dev",
                               "cpm_expected_grad_dest_batch"]

# every symbol include/cpm_expected_fit.h declares (checked by tests/test_expected_fit.py); a header and a list of its own, likewise
EXPECTED_FIT_SYMBOLS = ["cpm_set_measured_activity", "cpm_expected_fit_dev", "cpm_expected_fit"]

# every symbol include/cpm_expected_tangent.h declares (checked by tests/test_expected_tangent.py); a header and a list of its own, likewise
EXPECTED_TANGENT_SYMBOLS = ["cpm_expected_tangent_dev", "cpm_expected_tangent", "cpm_build_p_drive_tangent_dev", "cpm_build_p_drive_tangent"]
CPM_TANGENT_MAX_DIRECTIONS = 16  # K of one expected_tangent call

# every symbol include/cpm_expected_sparse.h declares (checked by tests/test_expected_sparse.py); a header and a list of its own, likewise
EXPECTED_SPARSE_SYMBOLS = ["cpm_expected_sparse_dev", "cpm_expected_sparse_batch_dev", "cpm_expected_sparse", "cpm_expected_sparse_batch",
                           "cpm_expected_sparse_aux"]

# every symbol include/cpm_expected_sparse_grad.h declares (checked by tests/test_expected_sparse_grad.py); a header and a list of its own, likewise
EXPECTED_SPARSE_GRAD_SYMBOLS = ["cpm_expected_sparse_grad_dev", "cpm_expected_sparse_grad", "cpm_expected_sparse_grad_batch_dev",
                                "cpm_expected_sparse_grad_batch", "cpm_expected_sparse_trip_dev", "cpm_expected_sparse_trip",
                                "cpm_expected_sparse_travel_dev", "cpm_expected_sparse_travel", "cpm_expected_sparse_travel_batch",
                                "cpm_expected_sparse_fit_dev", "cpm_expected_sparse_fit"]

# every symbol include/cpm_expected_sparse_dest.h declares (checked by tests/test_expected_sparse_dest.py); a header and a list of its own, likewise
EXPECTED_SPARSE_DEST_SYMBOLS = ["cpm_build_p_dest_tangent_sparse", "cpm_set_p_dest_tangent_sparse", "cpm_get_p_dest_tangent_sparse",
                                "cpm_expected_sparse_grad_dest_dev", "cpm_expected_sparse_grad_dest", "cpm_expected_sparse_grad_dest_batch_dev",
                                "cpm_expected_sparse_grad_dest_batch", "cpm_expected_sparse_trip_tangent_dev", "cpm_expected_sparse_trip_tangent"]
# its cpm_get_info keys: 1 while the dense tangent array is allocated and valid; 1 while a compact tangent is installed
CPM_INFO_DEST_TANGENT_DENSE, CPM_INFO_DEST_TANGENT_COMPACT = 25, 26

# every symbol include/cpm_expected_sparse_tangent.h declares (checked by tests/test_expected_sparse_tangent.py); a header and a list of its own, likewise
EXPECTED_SPARSE_TANGENT_SYMBOLS = ["cpm_expected_sparse_tangent_dev", "cpm_expected_sparse_tangent"]

# every symbol include/cpm_expected_var.h declares (checked by tests/test_expected_var.py); a header and a list of its own, likewise
EXPECTED_VAR_SYMBOLS = ["cpm_expected_var_dev", "cpm_expected_var"]
# every symbol include/cpm_expected_linear_var.h declares (checked by tests/test_expected_linear_var.py); likewise
EXPECTED_LINEAR_VAR_SYMBOLS = ["cpm_expected_linear_var_dev", "cpm_expected_linear_var"]
# every symbol include/cpm_expected_travel_var.h declares (checked by tests/test_expected_travel_var.py); likewise
EXPECTED_TRAVEL_VAR_SYMBOLS = ["cpm_expected_trip_var_dev", "cpm_expected_trip_var", "cpm_expected_trip_var_builds", "cpm_expected_travel_var_dev",
                               "cpm_expected_travel_var"]
# every symbol include/cpm_expected_sparse_var.h declares (checked by tests/test_expected_sparse_var.py); likewise
EXPECTED_SPARSE_VAR_SYMBOLS = ["cpm_expected_sparse_linear_var_dev", "cpm_expected_sparse_linear_var", "cpm_expected_sparse_trip_var_dev",
                               "cpm_expected_sparse_trip_var", "cpm_expected_sparse_trip_var_builds", "cpm_expected_sparse_travel_var_dev",
                               "cpm_expected_sparse_travel_var"]

CPM_FLAG_TRAVEL = 1
CPM_KERNEL_AUTO, CPM_KERNEL_CAR, CPM_KERNEL_ZONE_LDS = 0, 1, 2
CPM_KERNEL_ZONE_GROUPED = 5
CPM_OPT_KERNEL, CPM_OPT_PROFILE, CPM_OPT_PROFILE_KERNEL, CPM_OPT_FUSED, CPM_OPT_FUSED_LAG, CPM_OPT_ZONE_ORDER = 1, 2, 3, 4, 5, 6
CPM_OPT_SPARSE_UPLOAD = 7  # set_p_dest: sparse row packs for an uploaded p_destin that qualifies (include/cpm.h)
CPM_OPT_LAST_HOUR = 8  # hour T of a grouped resample: 1 (default) counts only where only its counts are wanted, 0 the plain sampler (include/cpm.h)
CPM_OPT_NARROW_PACK = 9  # the one-launch hour on dense packs in zone order: 1 (default) narrow row packs where the rule allows, 0 wide (include/cpm.h)
CPM_INFO_NARROW_PACK, CPM_INFO_NARROW_TIES = 14, 15  # 1: the last step's applied hours streamed narrow packs; the undecided draws so far (a blocking read)
CPM_OPT_FLOWS_KEPT = 16  # include/cpm_flows.h: the OD kernel once per resample over the kept runs of all hours (1) or once per hour (0, default)
CPM_PROFILE_SAMPLER, CPM_PROFILE_PLACE, CPM_PROFILE_TRAVEL, CPM_PROFILE_UPLOAD = 0, 1, 2, 3
# cpm_get_info keys (include/cpm.h): what the context would run next ...
CPM_INFO_KERNEL, CPM_INFO_CAP_MULT, CPM_INFO_PARTS, CPM_INFO_FUSED, CPM_INFO_FUSED_BAILOUTS, CPM_INFO_SPARSE_TABLES = 1, 2, 3, 4, 5, 6
# ... and what its most recent step ran
CPM_INFO_LAST_KERNEL, CPM_INFO_LAST_FORM, CPM_INFO_STEPS_REPEATED = 7, 8, 9
CPM_INFO_LAST_HOUR = 11  # 1: hour T of the most recent step ran the count-only kernel (10 stays unknown: tests/abi_harness.c)
CPM_INFO_TRAVEL_TABLE = 12  # the travel table of the resident datamatrix: 0 none yet, 1 compact rows (dataset route), 2 sparse rows, 3 dense gather
CPM_INFO_P_DENSE = 13  # 1: the dense [T][Z][Z] p_destin array is resident and valid for the installed tables (include/cpm.h)
CPM_KIT_LOG, CPM_KIT_SQRT, CPM_KIT_ERF, CPM_KIT_PPND, CPM_KIT_EXP_NEG = 0, 1, 2, 3, 4  # cpm_debug_f64_kit's functions
# include/cpm_batch.h: the installed batch tables' fleets, the fleets the batched kernels produced in the most recent batch step, and the
# CPM_INFO_LAST_FORM of such a step
CPM_MAX_BATCH = 64
CPM_INFO_BATCH, CPM_INFO_LAST_BATCH_FLEETS = 16, 17
CPM_FORM_BATCH = 10
# include/cpm.h: which instantiation the most recent step launched, one word per role (0: no such launch), written by the innermost
# launch helper from its template parameters: kind | CPT << 8 | NQ << 16 | flags << 24 (placing kinds: kind | KRUNS << 8 | PB / 64 << 16)
CPM_INFO_CELL_APPLIED, CPM_INFO_CELL_HEAVY, CPM_INFO_CELL_LAST, CPM_INFO_CELL_PLACE, CPM_INFO_CELL_BATCH = 20, 21, 22, 23, 24
CPM_CELL_SAMPLE, CPM_CELL_HOUR, CPM_CELL_HOUR_PF, CPM_CELL_DAY, CPM_CELL_HEAVY, CPM_CELL_COUNT, CPM_CELL_PLACE = 1, 2, 3, 4, 5, 6, 7
CPM_CELL_BATCH_SAMPLE, CPM_CELL_BATCH_PLACE, CPM_CELL_BATCH_COUNT = 8, 9, 10
CPM_CELL_FLAG_GROUPED, CPM_CELL_FLAG_SPARSE, CPM_CELL_FLAG_PERM = 1, 2, 4

_lib = None


class CpmError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"libcpm_hip status {status}: {message}")
        self.status = status


def build(force=False):
    """Compile libcpm_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) or f == "Makefile"]
    srcs.append(os.path.join(_HERE, "..", "include", "cpm.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_batch.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_flows.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_flows_csr.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_stays.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_paths.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_charge.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_objectives.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_travel.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_grad.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_grad_dest.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_grad_batch.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_fit.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_tangent.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_sparse.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_sparse_grad.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_sparse_dest.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_sparse_tangent.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_var.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_linear_var.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_travel_var.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "cpm_expected_sparse_var.h"))
    if (not force and os.path.exists(LIB_PATH)
            and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs)):
        return LIB_PATH
    subprocess.check_call(["make", "-C", CSRC, "libcpm_hip.so"] + (["-B"] if force else []))
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  carparkingmaps_amd has no CPU fallback.")
    # One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 / libhsa-runtime64 (same
    # SONAME as /opt/rocm's).  If this library is loaded first it pulls in the system copies, a later
    # `import torch` adds the bundled ones, and the second runtime's initialisation can fail ("No HIP
    # GPUs are available", seen after a long pytest session).  Importing torch first makes the dynamic
    # loader bind libcpm_hip.so to the copy that is already mapped.  Without torch (e.g. under the Julia
    # shim) the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    i32, i64, u32, u64, dbl, vp = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p
    L.cpm_last_error.restype = C.c_char_p
    L.cpm_version.restype = i32
    L.cpm_device_count.argtypes = [C.POINTER(i32)]
    L.cpm_device_info.argtypes = [i32, C.c_char_p, i32, C.POINTER(i32), C.POINTER(i64)]
    L.cpm_create.argtypes = [C.POINTER(vp), i64, i64, i32]
    L.cpm_destroy.argtypes = [vp]
    L.cpm_set_option.argtypes = [vp, i32, i64]
    L.cpm_set_stream.argtypes = [vp, vp]
    L.cpm_sync.argtypes = [vp]
    L.cpm_set_p_drive.argtypes = [vp, vp]
    L.cpm_set_p_dest.argtypes = [vp, vp]
    L.cpm_set_datamatrix.argtypes = [vp, vp, vp]
    L.cpm_build_p_drive.argtypes = [vp, dbl, dbl, dbl, vp]
    L.cpm_build_p_dest.argtypes = [vp, dbl, i32, vp]
    L.cpm_get_p_drive.argtypes = [vp, vp]
    L.cpm_get_cdf_row.argtypes = [vp, i64, i64, vp]
    L.cpm_init_states.argtypes = [vp, i64, i64, i64, i64]
    L.cpm_init_states_strided.argtypes = [vp, i64, i64, i64, i64, i64]
    L.cpm_set_state.argtypes = [vp, vp]
    L.cpm_get_state.argtypes = [vp, vp]
    L.cpm_solve_ivp.argtypes = [vp, u64, vp]
    L.cpm_resample.argtypes = [vp, u64, u32, vp, vp, vp, vp, vp]
    L.cpm_resample_dev.argtypes = [vp, u64, u32, vp]
    L.cpm_solve_ivp_async.argtypes = [vp, u64]
    L.cpm_synth_tables.argtypes = [vp, u64]
    L.cpm_synth_tables_skewed.argtypes = [vp, u64, i64]
    L.cpm_synth_datamatrix.argtypes = [vp, u64, dbl]
    L.cpm_refresh_tables.argtypes = [vp, i32]
    L.cpm_last_kernel_ms.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.cpm_algorithmic_bytes_per_hour.argtypes = [vp, C.POINTER(i64)]
    L.cpm_debug_categorical.argtypes = [vp, i64, i64, i64, vp, vp, C.POINTER(i32)]
    L.cpm_debug_travel_draw.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
    L.cpm_debug_f64_kit.argtypes = [vp, i32, i64, vp, vp]
    L.cpm_createdatamatrix_rows.argtypes = [vp, i64, vp]
    L.cpm_createdatamatrix_csv.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    L.cpm_get_datamatrix.argtypes = [vp, vp]
    L.cpm_parse_uber_csv.argtypes = [C.c_char_p, C.POINTER(i64), vp, i64]
    L.cpm_set_distance_from_centroids.argtypes = [vp, vp, vp]
    L.cpm_get_distance.argtypes = [vp, vp]
    L.cpm_set_distance.argtypes = [vp, vp]
    L.cpm_get_info.argtypes = [vp, i32, C.POINTER(i64)]
    L.cpm_set_p_drive_batch.argtypes = [vp, i32, vp]
    L.cpm_build_p_drive_batch.argtypes = [vp, i32, vp, vp, vp]
    L.cpm_get_p_drive_batch.argtypes = [vp, vp]
    L.cpm_resample_batch.argtypes = [vp, vp, u32, vp, vp, vp]
    L.cpm_resample_batch_dev.argtypes = [vp, vp, u32, vp]
    L.cpm_resample_flows.argtypes = [vp, u64, u32, vp, vp, vp, vp]
    L.cpm_resample_flows_dev.argtypes = [vp, u64, u32, vp, vp]
    L.cpm_resample_flows_csr_dev.argtypes = [vp, u64, u32, vp, vp, vp, vp, i64]
    L.cpm_resample_flows_csr.argtypes = [vp, u64, u32, vp, vp, vp, vp, C.POINTER(i64)]
    L.cpm_get_flows_csr.argtypes = [vp, vp, vp, i64]
    L.cpm_resample_stays.argtypes = [vp, u64, u32, vp, vp, vp, vp, vp]
    L.cpm_resample_stays_dev.argtypes = [vp, u64, u32, vp, vp, vp]
    L.cpm_resample_paths.argtypes = [vp, u64, u32, vp, vp, vp, vp]
    L.cpm_resample_paths_dev.argtypes = [vp, u64, u32, vp, vp]
    L.cpm_paths_expand_dev.argtypes = [vp, u64, u32, vp, vp, vp]
    L.cpm_resample_charge.argtypes = [vp, u64, u32, C.POINTER(ChargeParamsC), vp, vp, vp, vp, vp, vp, vp]
    L.cpm_resample_charge_dev.argtypes = [vp, u64, u32, C.POINTER(ChargeParamsC), vp, vp, vp, vp, vp]
    L.cpm_set_measured.argtypes = [vp, vp]
    L.cpm_objectives_dev.argtypes = [vp, vp, i32, i64, vp, vp]
    L.cpm_expected_dev.argtypes = [vp, vp, u32, vp, vp]
    L.cpm_expected_batch_dev.argtypes = [vp, vp, u32, vp]
    L.cpm_expected.argtypes = [vp, vp, u32, vp, vp, vp]
    L.cpm_expected_batch.argtypes = [vp, vp, u32, vp, vp]
    L.cpm_expected_sparse_dev.argtypes = [vp, vp, u32, vp, vp]
    L.cpm_expected_sparse_batch_dev.argtypes = [vp, vp, u32, vp]
    L.cpm_expected_sparse.argtypes = [vp, vp, u32, vp, vp, vp]
    L.cpm_expected_sparse_batch.argtypes = [vp, vp, u32, vp, vp]
    L.cpm_expected_sparse_aux.argtypes = [vp, i32, vp, vp, vp, vp]
    L.cpm_expected_sparse_grad_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.cpm_expected_sparse_grad.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_grad_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.cpm_expected_sparse_grad_batch.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_trip_dev.argtypes = [vp, vp]
    L.cpm_expected_sparse_trip.argtypes = [vp, vp, vp]
    L.cpm_expected_sparse_travel_dev.argtypes = [vp, vp, i32, vp, vp]
    L.cpm_expected_sparse_travel.argtypes = [vp, vp, u32, vp, vp, vp]
    L.cpm_expected_sparse_travel_batch.argtypes = [vp, vp, u32, vp, vp, vp]
    L.cpm_expected_sparse_fit_dev.argtypes = [vp, i32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_fit.argtypes = [vp, i32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_build_p_dest_tangent_sparse.argtypes = [vp]
    L.cpm_set_p_dest_tangent_sparse.argtypes = [vp, vp]
    L.cpm_get_p_dest_tangent_sparse.argtypes = [vp, vp]
    L.cpm_expected_sparse_grad_dest_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_grad_dest.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_grad_dest_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_grad_dest_batch.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_trip_tangent_dev.argtypes = [vp, vp]
    L.cpm_expected_sparse_trip_tangent.argtypes = [vp, vp, vp]
    L.cpm_expected_trip_dev.argtypes = [vp, vp]
    L.cpm_expected_trip.argtypes = [vp, vp, vp]
    L.cpm_expected_travel_dev.argtypes = [vp, vp, i32, vp, vp]
    L.cpm_expected_travel.argtypes = [vp, vp, u32, vp, vp, vp]
    L.cpm_expected_travel_batch.argtypes = [vp, vp, u32, vp, vp, vp]
    L.cpm_expected_trip_builds.argtypes = [vp]
    L.cpm_expected_grad_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.cpm_expected_grad.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_set_p_dest_tangent.argtypes = [vp, vp]
    L.cpm_build_p_dest_tangent.argtypes = [vp, vp]
    L.cpm_get_p_dest_tangent.argtypes = [vp, vp]
    L.cpm_expected_grad_dest_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_expected_grad_dest.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_trip_tangent_dev.argtypes = [vp, vp]
    L.cpm_expected_trip_tangent.argtypes = [vp, vp, vp]
    L.cpm_expected_grad_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.cpm_expected_grad_batch.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_expected_grad_dest_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    L.cpm_expected_grad_dest_batch.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_set_measured_activity.argtypes = [vp, vp]
    L.cpm_expected_fit_dev.argtypes = [vp, i32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_fit.argtypes = [vp, i32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_tangent_dev.argtypes = [vp, i32, vp, u32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_tangent.argtypes = [vp, i32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_tangent_dev.argtypes = L.cpm_expected_tangent_dev.argtypes
    L.cpm_expected_sparse_tangent.argtypes = L.cpm_expected_tangent.argtypes
    L.cpm_build_p_drive_tangent_dev.argtypes = [vp, dbl, dbl, dbl, vp]
    L.cpm_build_p_drive_tangent.argtypes = [vp, dbl, dbl, dbl, vp]
    L.cpm_expected_var_dev.argtypes = [vp, vp, u32, vp]
    L.cpm_expected_var.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.cpm_expected_linear_var_dev.argtypes = [vp, vp, u32, i32, vp, vp, vp]
    L.cpm_expected_linear_var.argtypes = [vp, vp, u32, i32, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_trip_var_dev.argtypes = [vp, vp]
    L.cpm_expected_trip_var.argtypes = [vp, vp]
    L.cpm_expected_trip_var_builds.argtypes = [vp]
    L.cpm_expected_travel_var_dev.argtypes = [vp, vp, u32, i32, vp, vp, vp]
    L.cpm_expected_travel_var.argtypes = [vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cpm_expected_sparse_linear_var_dev.argtypes = L.cpm_expected_linear_var_dev.argtypes
    L.cpm_expected_sparse_linear_var.argtypes = L.cpm_expected_linear_var.argtypes
    L.cpm_expected_sparse_trip_var_dev.argtypes = L.cpm_expected_trip_var_dev.argtypes
    L.cpm_expected_sparse_trip_var.argtypes = L.cpm_expected_trip_var.argtypes
    L.cpm_expected_sparse_trip_var_builds.argtypes = L.cpm_expected_trip_var_builds.argtypes
    L.cpm_expected_sparse_travel_var_dev.argtypes = L.cpm_expected_travel_var_dev.argtypes
    L.cpm_expected_sparse_travel_var.argtypes = L.cpm_expected_travel_var.argtypes
    for name in (SYMBOLS + BATCH_SYMBOLS + FLOWS_SYMBOLS + FLOWS_CSR_SYMBOLS + STAYS_SYMBOLS + PATHS_SYMBOLS + CHARGE_SYMBOLS + OBJECTIVES_SYMBOLS
                 + EXPECTED_SYMBOLS + EXPECTED_TRAVEL_SYMBOLS + EXPECTED_GRAD_SYMBOLS + EXPECTED_GRAD_DEST_SYMBOLS + EXPECTED_GRAD_BATCH_SYMBOLS
                 + EXPECTED_FIT_SYMBOLS + EXPECTED_TANGENT_SYMBOLS + EXPECTED_SPARSE_SYMBOLS + EXPECTED_SPARSE_GRAD_SYMBOLS
                 + EXPECTED_SPARSE_DEST_SYMBOLS + EXPECTED_SPARSE_TANGENT_SYMBOLS + EXPECTED_VAR_SYMBOLS + EXPECTED_LINEAR_VAR_SYMBOLS
                 + EXPECTED_TRAVEL_VAR_SYMBOLS + EXPECTED_SPARSE_VAR_SYMBOLS):
        fn = getattr(L, name)
        if name not in ("cpm_last_error",):
            fn.restype = i32
    L.cpm_expected_trip_builds.restype = i64  # (a counter; negative: a status code)
    L.cpm_expected_trip_var_builds.restype = i64
    L.cpm_expected_sparse_trip_var_builds.restype = i64
    _lib = L
    return L


def check(status):
    if status != 0:
        raise CpmError(status, load().cpm_last_error().decode("utf-8", "replace"))
