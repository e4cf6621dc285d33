"""The batched resample's host side without a GPU: include/cpm_batch.h against the loader and the library, argument errors, the
header under a strict C compiler, and the model-selection sweep's cutting of a lane's points into batches."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT


def _declared_batch():
    text = open(os.path.join(ROOT, "include", "cpm_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def test_batch_header_declares_exactly_the_batch_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared_batch()
    assert declared and sorted(_lib.BATCH_SYMBOLS) == declared
    assert not set(declared) & set(_lib.SYMBOLS)           # cpm.h's list is untouched
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_batch.h but not exported"


def test_batch_constants_match_the_header(cpm):
    from carparkingmaps_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpm_batch.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define (CPM_\w+) (\d+)", text)}
    assert got == {"CPM_MAX_BATCH": _lib.CPM_MAX_BATCH, "CPM_INFO_BATCH": _lib.CPM_INFO_BATCH,
                   "CPM_INFO_LAST_BATCH_FLEETS": _lib.CPM_INFO_LAST_BATCH_FLEETS, "CPM_FORM_BATCH": _lib.CPM_FORM_BATCH}
    # the key behind CPM_INFO_STEPS_REPEATED stays unknown (tests/abi_harness.c pins it)
    assert _lib.CPM_INFO_STEPS_REPEATED + 1 not in (_lib.CPM_INFO_BATCH, _lib.CPM_INFO_LAST_BATCH_FLEETS)


def test_null_context_and_batch_size_out_of_range_are_argument_errors(cpm):
    from carparkingmaps_amd import _lib
    import numpy as np
    L = _lib.load()
    ERR_ARG = -1
    p = np.zeros(4, dtype=np.float64)
    vp = p.ctypes.data_as(ctypes.c_void_p)
    seeds = np.zeros(4, dtype=np.uint64).ctypes.data_as(ctypes.c_void_p)
    for B in (1, 0, -1, _lib.CPM_MAX_BATCH + 1):
        assert L.cpm_set_p_drive_batch(None, B, vp) == ERR_ARG
        assert L.cpm_build_p_drive_batch(None, B, vp, vp, vp) == ERR_ARG
    assert L.cpm_get_p_drive_batch(None, vp) == ERR_ARG
    assert L.cpm_resample_batch(None, seeds, 0, vp, vp, None) == ERR_ARG
    assert L.cpm_resample_batch_dev(None, seeds, 0, vp) == ERR_ARG
    assert b"null context" in L.cpm_last_error()


def test_batch_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "batch_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_batch.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    uint64_t seeds[CPM_MAX_BATCH] = {0};
    double p[4] = {0};
    int64_t counts[4] = {0};
    int32_t rc = cpm_set_p_drive_batch(ctx, 1, p) + cpm_build_p_drive_batch(ctx, 1, p, p, p) + cpm_get_p_drive_batch(ctx, p) +
                 cpm_resample_batch(ctx, seeds, CPM_FLAG_TRAVEL, counts, counts, NULL) + cpm_resample_batch_dev(ctx, seeds, 0u, counts);
    return (rc == 5 * CPM_ERR_ARG && CPM_INFO_BATCH != CPM_INFO_LAST_BATCH_FLEETS && CPM_FORM_BATCH == 10) ? 0 : 1;
}
""")
    exe = str(tmp_path / "batch_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.run([exe]).returncode == 0


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("B", [1, 4, 5, 64])
def test_batch_cuts_of_the_sweep(world, lanes, B):
    """Every point of a lane lands in exactly one batch, a batch holds one e_dest and at most B points, and the lane's order is kept."""
    from carparkingmaps_amd import model_selection as ms
    grid = ms.make_grid()
    by_e_dest = sorted(range(len(grid)), key=lambda i: (float(grid[i].e_dest), type(grid[i].e_dest).__name__, i))
    seen = []
    for rank in range(world):
        mine = ms.points_of_rank(len(grid), rank, world, by_e_dest)
        for lane in range(lanes):
            pts = ms.points_of_rank(len(mine), lane, lanes, mine)
            cuts = ms.batch_cuts(grid, pts, B)
            assert [i for c in cuts for i in c] == pts
            for c in cuts:
                assert 1 <= len(c) <= B
                assert len({ms.e_dest_key(grid[i].e_dest) for i in c}) == 1
            # as few batches as the e_dest runs allow: only the last batch of an e_dest run may be short
            for a, b in zip(cuts, cuts[1:]):
                if ms.e_dest_key(grid[a[0]].e_dest) == ms.e_dest_key(grid[b[0]].e_dest):
                    assert len(a) == B
            seen += pts
    assert sorted(seen) == list(range(len(grid)))


def test_batch_cuts_tell_integer_and_float_exponents_apart():
    from carparkingmaps_amd import model_selection as ms
    grid = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(1.0, 0.1, 0.9, 2), ms.Point(0.5, 0.1, 0.9, 2.0), ms.Point(1.0, 0.1, 0.9, 2.0)]
    assert ms.batch_cuts(grid, [0, 1, 2, 3], 8) == [[0, 1], [2, 3]]
