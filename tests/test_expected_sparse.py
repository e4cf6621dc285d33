"""The expected densities from sparse tables (include/cpm_expected_sparse.h) without a GPU: the lane rule of the header against a
brute-force walk of exp_stream's loop indices; one hourly product in the dense kernel's order against the same in the sparse kernel's
order, bit for bit, on tables with a column of every origin, empty columns, zero rows, rows below 1, a stored cell of weight 0 and
zeros in pi; a mutant order that must differ; and the host side of the new entries."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import expected_sparse_reference as S

ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_expected_sparse_dev", "cpm_expected_sparse_batch_dev", "cpm_expected_sparse", "cpm_expected_sparse_batch", "cpm_expected_sparse_aux"]
SIZES = [2, 3, 4, 5, 511, 512, 513, 514, 1030, 1031]
T = 2                                   # hours 0 and 1: both alignments of an odd Z's rows occur at every destination


# ------------------------------------------------------------------ the lane rule
@pytest.mark.parametrize("Z", SIZES + [1536, 1537])
def test_key_rule_is_the_walk_of_the_dense_kernels_loops(Z):
    for hd in ((False, True) if Z & 1 else (False,)):
        walk = S.brute_walk(Z, hd)
        assert sorted(o for seq in walk for o in seq) == list(range(Z))          # every origin once
        keys = sorted((S.lane_key(o, Z, hd), o) for o in range(Z))
        by_key = [[] for _ in range(S.LANES)]
        for (lane, _), o in keys:
            by_key[lane].append(o)
        assert by_key == walk, (Z, hd)


def test_head_alternates_with_hour_and_destination_for_odd_z_only():
    for Z in (4, 512):
        assert not any(S.head(Z, t, d) for t in range(3) for d in range(Z))
    for Z in (3, 513, 1031):
        for t in range(3):
            for d in range(Z):
                assert S.head(Z, t, d) == (((t + d) & 1) == 1)


def test_the_wave_tree_is_the_shuffle_tree():
    v = np.random.default_rng(1).random(64)
    w = list(v)
    for o in (32, 16, 8, 4, 2, 1):
        w = [w[i] + (w[i + o] if i + o < 64 else w[i]) for i in range(64)]
    assert S.wave_tree(v) == w[0]


# ------------------------------------------------------------------ dense order == sparse order
def _case(Z):
    p_drive, p_dest, info = S.sparse_tables(Z, T)
    return p_drive, p_dest, info, S.pi0_with_zeros(Z)


@pytest.mark.parametrize("Z", SIZES)
def test_sparse_order_gives_the_bits_of_the_dense_order(Z):
    p_drive, p_dest, info, pi = _case(Z)
    for t in range(T):
        p_t = np.ascontiguousarray(p_dest[:, :, t])
        if t == T - 1:
            assert (p_t[:, info["full"]] > 0).all(), "a column holding every origin"
        else:
            assert all(not p_t[o].any() for o in info["zero"])
        assert all(not p_t[:, d].any() for d in info["empty"])
        if Z > 2:
            assert (S.row_last(p_t)[info["half"]] < 0.75).all()
        # cells of weight 0 that stay stored (the dataset route keeps them): some in front of, some behind a row's last positive cell
        zeros = np.argwhere(p_t == 0.0)
        keep = [tuple(c) for c in zeros[:: max(1, len(zeros) // 50)]] + [(Z - 1, Z - 1), (0, Z - 1)]
        dense = S.dense_hour(p_t, pi, p_drive[:, t], t)
        sparse = S.sparse_hour(p_t, pi, p_drive[:, t], t, keep_zero=keep)
        assert np.array_equal(dense, sparse), (Z, t)
        assert np.array_equal(np.signbit(dense), np.signbit(sparse))
        assert dense.sum() > 0
        pi = dense                                                   # hour 1 starts from hour 0's result


def test_a_column_sorted_without_the_lane_wrap_differs():
    """the cases can tell: at Z = 1,031 origins >= 512 wrap into lanes that already hold cells"""
    Z = 1031
    p_drive, p_dest, info, pi = _case(Z)
    differs = False
    for t in range(T):
        p_t = np.ascontiguousarray(p_dest[:, :, t])
        dense = S.dense_hour(p_t, pi, p_drive[:, t], t)
        mutant = S.sparse_hour(p_t, pi, p_drive[:, t], t, key=S.mutant_key)
        differs = differs or not np.array_equal(dense, mutant)
        np.testing.assert_allclose(mutant, dense, rtol=1e-12)       # (the same sums in another order)
    assert differs


def test_below_the_wrap_the_mutant_is_the_rule():
    for Z in (4, 5, 511, 512):
        for hd in ((False, True) if Z & 1 else (False,)):
            assert all(S.mutant_key(o, Z, hd) == S.lane_key(o, Z, hd) for o in range(Z))
    assert any(S.mutant_key(o, 1031, False) != S.lane_key(o, 1031, False) for o in range(1031))


# ------------------------------------------------------------------ host side
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_sparse.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_SPARSE_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "EXPECTED_SPARSE_SYMBOLS"]
    assert len(others) >= 15
    for other in others:
        assert not set(declared) & set(other)
    L = _lib.load()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_sparse.h but not exported"
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int32
    text = open(os.path.join(ROOT, "include", "cpm_expected_sparse.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_SPARSE_H"]      # no option, info key, status or flag of its own
    assert '#include "cpm_expected.h"' in text
    for h in os.listdir(os.path.join(ROOT, "include")):                              # included from nothing existing
        if h != "cpm_expected_sparse.h":
            assert '#include "cpm_expected_sparse.h"' not in open(os.path.join(ROOT, "include", h)).read()
    import inspect
    for method in ("expected", "expected_batch", "expected_dev", "expected_batch_dev"):
        assert inspect.signature(getattr(cpm.Sampler, method)).parameters["sparse"].default is False
    from carparkingmaps_amd.model_selection import Evaluator
    assert Evaluator.__dataclass_fields__["expected_sparse"].default is False


def test_the_new_info_number_is_distinct_from_all_existing_ones(cpm):
    from carparkingmaps_amd import _lib
    numbers = {}
    for h in os.listdir(os.path.join(ROOT, "include")):
        for name, num in re.findall(r"#define\s+(CPM_INFO_\w+)\s+(\d+)", open(os.path.join(ROOT, "include", h)).read()):
            assert name not in numbers
            numbers[name] = int(num)
    assert numbers["CPM_INFO_P_DENSE"] == _lib.CPM_INFO_P_DENSE == cpm.CPM_INFO_P_DENSE
    assert len(set(numbers.values())) == len(numbers) and len(numbers) >= 19
    assert numbers["CPM_INFO_P_DENSE"] != 10                                        # (10 stays unknown: tests/abi_harness.c)
    py = {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("CPM_INFO_")}
    assert py == {k: numbers[k] for k in py}


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_sparse_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_sparse.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[4] = {0};
    int32_t b[4] = {0};
    int32_t r[5];
    int i;
    r[0] = cpm_expected_sparse_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL);
    r[1] = cpm_expected_sparse_batch_dev(ctx, NULL, 0u, a);
    r[2] = cpm_expected_sparse(ctx, NULL, 0u, a, a, NULL);
    r[3] = cpm_expected_sparse_batch(ctx, NULL, CPM_EXPECT_IVP, a, a);
    r[4] = cpm_expected_sparse_aux(ctx, 1, b, a, b, b);
    for (i = 1; i < 5; ++i) if (r[i] != r[0]) return 1;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_sparse_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    probe = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); n = ctypes.c_int32(0); "
             "sys.exit(0 if L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1 else 2)")
    want = subprocess.run([sys.executable, "-c", probe, _lib.LIB_PATH]).returncode
    assert want in (0, 2) and subprocess.run([exe]).returncode == want


def test_every_entry_returns_err_hip_without_a_device(cpm):
    from carparkingmaps_amd import _lib
    L = _lib.load()
    a = np.zeros(32)
    vp = a.ctypes.data_as(ctypes.c_void_p)
    want = ERR_HIP if _no_device(L) else ERR_ARG
    for flags in (0, _lib.CPM_EXPECT_IVP):
        assert L.cpm_expected_sparse_dev(None, None, flags, vp, None) == want
        assert L.cpm_expected_sparse_batch_dev(None, None, flags, vp) == want
        assert L.cpm_expected_sparse(None, None, flags, vp, vp, None) == want
        assert L.cpm_expected_sparse_batch(None, None, flags, vp, vp) == want
    assert L.cpm_expected_sparse_aux(None, 1, vp, vp, vp, vp) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()
