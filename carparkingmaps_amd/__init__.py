"""carparkingmaps_amd -- MI355X (gfx950) implementation of the CarParkingMaps HMM traffic-flow
sampler path (initializestates -> solveinitialvalueproblem -> resampling -> zone x hour
histogram, fed by the p_drive / p_dest tables), behind the reference's own call surface.

The compute lives in csrc/libcpm_hip.so (hand-written HIP, C ABI in include/cpm.h).  There is
no CPU fallback; importing the package works without a GPU, computing does not.
"""
from . import _lib
from ._lib import (CPM_FORM_BATCH, CPM_INFO_BATCH, CPM_INFO_LAST_BATCH_FLEETS, CPM_MAX_BATCH, CPM_INFO_CAP_MULT, CPM_INFO_FUSED, CPM_INFO_FUSED_BAILOUTS, CPM_INFO_KERNEL, CPM_INFO_LAST_FORM, CPM_INFO_LAST_HOUR,
                   CPM_INFO_LAST_KERNEL, CPM_INFO_PARTS, CPM_INFO_SPARSE_TABLES, CPM_INFO_STEPS_REPEATED, CPM_INFO_TRAVEL_TABLE, CPM_INFO_P_DENSE, CPM_KERNEL_AUTO,
                   CPM_KERNEL_CAR, CPM_KERNEL_ZONE_GROUPED, CPM_KERNEL_ZONE_LDS, CpmError)
from ._lib import CPM_INFO_CELL_APPLIED, CPM_INFO_CELL_BATCH, CPM_INFO_CELL_HEAVY, CPM_INFO_CELL_LAST, CPM_INFO_CELL_PLACE
from ._lib import CPM_INFO_NARROW_PACK, CPM_INFO_NARROW_TIES
from .sampler import ChargeParams, Sampler, device_count, device_info, flows_csr_hour, flows_csr_to_dense, paths_flows, paths_to_matrices, stay_length_histogram
from .reference_api import (DeviceArray, Params, averagedrivingtime, correctparameters, createdatamatrix, createpdestin,
                            createpdrive, createresultsdirectory, initializestates, invalidate, params, processgeodata, release,
                            resampling, run_dataset, save_flows_csv, saveparameters, saveresults, solveinitialvalueproblem,
                            zone_hour_counts)

__all__ = [
    "Sampler", "ChargeParams", "device_count", "device_info", "CpmError", "CPM_KERNEL_AUTO", "CPM_KERNEL_CAR",
    "CPM_KERNEL_ZONE_LDS", "CPM_KERNEL_ZONE_GROUPED", "CPM_INFO_KERNEL", "CPM_INFO_CAP_MULT", "CPM_INFO_PARTS", "CPM_INFO_FUSED",
    "CPM_INFO_FUSED_BAILOUTS", "CPM_INFO_SPARSE_TABLES", "CPM_INFO_LAST_KERNEL", "CPM_INFO_LAST_FORM", "CPM_INFO_LAST_HOUR", "CPM_INFO_STEPS_REPEATED", "CPM_INFO_TRAVEL_TABLE", "CPM_INFO_P_DENSE", "CPM_INFO_BATCH", "CPM_INFO_LAST_BATCH_FLEETS", "CPM_INFO_CELL_APPLIED", "CPM_INFO_CELL_HEAVY", "CPM_INFO_CELL_LAST", "CPM_INFO_CELL_PLACE", "CPM_INFO_CELL_BATCH", "CPM_INFO_NARROW_PACK", "CPM_INFO_NARROW_TIES", "CPM_FORM_BATCH", "CPM_MAX_BATCH", "Params", "params", "createpdrive", "createpdestin", "initializestates",
    "solveinitialvalueproblem", "resampling", "averagedrivingtime", "correctparameters", "saveresults",
    "zone_hour_counts", "run_dataset", "release", "createdatamatrix", "processgeodata", "createresultsdirectory",
    "saveparameters", "DeviceArray", "invalidate", "flows_csr_to_dense", "flows_csr_hour", "save_flows_csv", "stay_length_histogram", "paths_to_matrices", "paths_flows",
]
