"""The forward tangent from the compact rows of sparse tables (include/cpm_expected_sparse_tangent.h), without a GPU: one operator of
k_tan_hour restated in numpy with every origin of the dense rows of p and dP, zeros included, against the order of k_exps_tan_hour over
the stored cells alone -- equal in every bit and in the sign of every zero, for SIGNED dx and for u on the masked primal; two mutants
that must differ; the header, the exports and the refusals that need no device."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import expected_sparse_reference as S
import expected_sparse_tangent_reference as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 403, 518, 1031, 1089]
TC = 2
NEW = ["cpm_expected_sparse_tangent", "cpm_expected_sparse_tangent_dev"]
WORDS = ("pi_next", "x_next", "dpi_next", "dx_next", "y", "dy", "u")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(np.signbit(a), np.signbit(b))


def _run(order, case, t, pi, dpi, dq, c, **kw):
    h = case["hours"][t]
    q = case["p_drive"]
    tn = (t + 1) % TC
    return ST.operator(order, h["p_t"], h["dP_t"], h["cols"], h["dcols"], pi, dpi, q[:, t], None if dq is None else dq[:, t], c, t,
                       q[:, tn], None if dq is None else dq[:, tn], **kw)


def test_the_cases_hold_what_they_are_meant_to():
    for Z in (403, 1089):
        case = ST.order_case(Z, TC)
        info, (dc, o1, o2) = case["info"], case["cancel"]
        for t, h in enumerate(case["hours"]):
            p_t, dP_t, stored = h["p_t"], h["dP_t"], h["stored"]
            assert (dP_t < 0).any() and (dP_t > 0).any() and not dP_t[~stored].any() and not np.signbit(dP_t[~stored]).any()
            assert all(p_t[o, d] == 0.0 and dP_t[o, d] != 0.0 for o, d in h["keep"])          # kept cells of weight 0 carry a tangent
            assert len(h["cols"][info["full"]]) == (Z if t == TC - 1 else Z - len(info["zero"]))   # a column of every origin (last hour)
            assert not h["cols"][case["empty"]] and not p_t[:, case["empty"]].any()            # an empty column
            assert sorted(o for o, _ in h["cols"][dc]) == [o1, o2] and p_t[o1, dc] == p_t[o2, dc]
            assert all([o for o, _ in a] == [o for o, _ in b] for a, b in zip(h["cols"], h["dcols"]))   # cell_dp entry for entry with cell_p
            rows = S.row_last(p_t)
            assert (rows < 0.75).any() and (rows <= 1.0).all()                                 # rows below 1
            zero_with_kept = [o for o in info["zero"] if not p_t[o].any() and any(oo == o for oo, _ in h["keep"])]
            assert (t == TC - 1) or len(zero_with_kept) == len(info["zero"]) > 0               # zero rows keep a cell with a tangent
        assert (case["pi"] == 0).any() and all(case["pi"][o] > 0 for o in info["zero"])
        assert (case["p_drive"][:, TC - 1] > 0).all() and (case["p_drive"][:, 0] == 0).any() and (case["p_drive"] == 1).any()
        names = [d[0] for d in ST.order_directions(case, Z, TC)]
        assert names == ["signed", "cancel", "negative"]
    assert max(len(c) for c in ST.order_case(1089, TC)["hours"][0]["cols"]) > 1024             # the lane wrap above 512, twice


@pytest.mark.parametrize("Z", SIZES)
def test_sparse_order_of_the_operator_gives_the_bits_of_the_dense_order(Z):
    case = ST.order_case(Z, TC)
    for name, dpi, dq, c in ST.order_directions(case, Z, TC):
        for t in range(TC):
            dense = _run("dense", case, t, case["pi"], dpi, dq, c)
            sparse = _run("sparse", case, t, case["pi"], dpi, dq, c)
            for k in WORDS:
                if dense[k] is None:
                    assert sparse[k] is None and c == 0.0
                    continue
                assert _bits_equal(dense[k], sparse[k]), (Z, name, t, k)
            for k in ("y", "dy", "u"):                                                         # an accumulator never becomes -0
                if dense[k] is not None:
                    assert not np.signbit(dense[k][dense[k] == 0.0]).any(), (Z, name, t, k)
            if name == "signed" and Z > 2:
                assert (dense["dy"] < 0).any() and (dense["dy"] > 0).any() and (dense["u"] != 0).any()
            if name == "cancel" and case["cancel"]:
                dc, o1, o2 = case["cancel"]
                x = dpi * S.exp_q(case["p_drive"][:, t])
                assert x[o1] == -x[o2] != 0.0
                assert dense["dy"][dc] == 0.0 and not np.signbit(dense["dy"][dc]) and not np.signbit(sparse["dy"][dc])   # exact cancellation: +0
            if name == "negative":
                dx = dpi * S.exp_q(case["p_drive"][:, t])
                assert (dx <= 0).all() and (t != TC - 1 or (dx < 0).all())                      # every dx negative (last hour: no q = 0)
                e = case["empty"]
                if e is not None:                                                              # dense: +0 + -0 + ... = +0; sparse: no cell
                    assert dense["dy"][e] == 0.0 and not np.signbit(dense["dy"][e]) and not np.signbit(sparse["dy"][e])
                if Z > 2:
                    assert (dense["dy"] < 0).any() and not (dense["dy"] > 0).any()


@pytest.mark.parametrize("Z", SIZES)
def test_an_hour_of_zero_pi_gives_the_same_bits_and_exact_zeros(Z):
    case = ST.order_case(Z, TC)
    _, dpi, dq, c = ST.order_directions(case, Z, TC)[0]
    zero = np.zeros(Z)
    dense, sparse = _run("dense", case, 0, zero, dpi, dq, c), _run("sparse", case, 0, zero, dpi, dq, c)
    for k in WORDS:
        assert _bits_equal(dense[k], sparse[k]), (Z, k)
    for k in ("pi_next", "x_next", "y", "u"):                                                  # the primal and u: +0 everywhere
        assert not dense[k].any() and not np.signbit(dense[k]).any(), k
    assert dense["dpi_next"].any()                                                             # dx = dpi * q still moves


def test_mutants_differ_at_every_size_where_they_can():
    for Z in SIZES:
        case = ST.order_case(Z, TC)
        _, dpi, dq, c = ST.order_directions(case, Z, TC)[0]
        good = _run("sparse", case, 0, case["pi"], dpi, dq, c)
        # the lanes do not wrap: origins past 511 stay in lane 255.  Below 512 origins the two keys are one
        wrap = _run("sparse", case, 0, case["pi"], dpi, dq, c, key=S.mutant_key)
        same = all(_bits_equal(good[k], wrap[k]) for k in WORDS)
        assert same == (Z <= 512), Z
        if not same:
            assert not _bits_equal(good["dy"], wrap["dy"]) and not _bits_equal(good["u"], wrap["u"]), Z
            scale = np.abs(dpi).max() * 4.0
            assert np.abs(good["dpi_next"] - wrap["dpi_next"]).max() <= 1e-12 * scale          # another order of the same sum
        # u on x instead of xm: differs where a zero row keeps a cell that carries a tangent
        on_x = _run("sparse", case, 0, case["pi"], dpi, dq, c, u_on="x")
        zero_rows = [o for o in case["info"]["zero"] if not case["hours"][0]["p_t"][o].any()]
        assert bool(zero_rows) == (Z > 2)
        if zero_rows:
            hit = sorted({d for o, d in case["hours"][0]["keep"] if o in zero_rows})
            diff = np.nonzero(good["u"] != on_x["u"])[0]
            assert hit and sorted(diff) == hit, Z
            assert not _bits_equal(good["dpi_next"], on_x["dpi_next"])
            assert _bits_equal(_run("dense", case, 0, case["pi"], dpi, dq, c, u_on="x")["u"], on_x["u"])
        else:
            assert _bits_equal(good["u"], on_x["u"])


# ------------------------------------------------------------------ host side
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_sparse_tangent.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_SPARSE_TANGENT_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "EXPECTED_SPARSE_TANGENT_SYMBOLS"]
    assert len(others) >= 18
    for other in others:
        assert not set(declared) & set(other)
    L = _lib.load()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_sparse_tangent.h but not exported"
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int32
    assert L.cpm_expected_sparse_tangent_dev.argtypes == L.cpm_expected_tangent_dev.argtypes
    assert L.cpm_expected_sparse_tangent.argtypes == L.cpm_expected_tangent.argtypes
    text = open(os.path.join(ROOT, "include", "cpm_expected_sparse_tangent.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_SPARSE_TANGENT_H"]
    assert '#include "cpm_expected_tangent.h"' in text and '#include "cpm_expected_sparse_dest.h"' in text
    for word in ("Why the bits agree", "never -0.0", "xm", "finite", "CPM_INFO_P_DENSE", "CPM_INFO_DEST_TANGENT_DENSE", "CPM_INFO_DEST_TANGENT_COMPACT",
                 "CPM_INFO_SPARSE_TABLES", "off the stored cells", "CPM_ERR_TABLE"):
        assert word in text, word
    for method in ("expected_tangent", "expected_tangent_dev"):
        assert inspect.signature(getattr(cpm.Sampler, method)).parameters["sparse"].default is False, method


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_sparse_tangent_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_sparse_tangent.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[8] = {0};
    int32_t r[2];
    r[0] = cpm_expected_sparse_tangent_dev(ctx, 1, NULL, CPM_EXPECT_IVP, NULL, NULL, a, a, NULL, NULL);
    r[1] = cpm_expected_sparse_tangent(ctx, CPM_TANGENT_MAX_DIRECTIONS, NULL, 0u, NULL, NULL, NULL, a, a, NULL, NULL, NULL);
    if (r[1] != r[0]) return 1;
    if (CPM_INFO_DEST_TANGENT_DENSE == CPM_INFO_DEST_TANGENT_COMPACT) return 4;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_sparse_tangent_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    probe = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); n = ctypes.c_int32(0); "
             "sys.exit(0 if L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1 else 2)")
    want = subprocess.run([sys.executable, "-c", probe, _lib.LIB_PATH]).returncode
    assert want in (0, 2) and subprocess.run([exe]).returncode == want


class _NoDevice:
    """a Sampler whose library must not be reached"""
    Z, T = 4, 2

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came too late: {name} was touched")


def test_python_refusals_come_before_any_device_call(cpm):
    from carparkingmaps_amd import model_selection as M
    with pytest.raises(ValueError, match="expected_sparse=True"):
        M.Evaluator(_NoDevice(), 1, 1, expected_sparse_tangent=True)
    with pytest.raises(ValueError, match="expected_sparse=True"):
        M.Evaluator(_NoDevice(), 1, 1, expected_sparse_dest=True, expected_sparse_tangent=True)
    ev = M.Evaluator(_NoDevice(), 1, 1, expected_sparse=True, expected_sparse_tangent=True)
    with pytest.raises(ValueError, match="expected_sparse_dest=True"):
        ev.expected_jacobian(M.Point(0.5, 0.1, 0.9, 2), dest=True)
    assert M.Evaluator(_NoDevice(), 1, 1).expected_sparse_tangent is False
    assert M.Evaluator(_NoDevice(), 1, 1, expected_sparse=True, expected_sparse_dest=True).expected_sparse_tangent is False
    for doc in (inspect.getdoc(M.Evaluator.expected_jacobian), inspect.getdoc(M.refine_expected_lm), inspect.getdoc(M.Evaluator)):
        assert "dense tangent" in doc.lower() and "expected_sparse_tangent" in doc
