"""The adjoint of the expected densities along a tangent of p_destin (include/cpm_expected_grad_dest.h), without a GPU: the ABI list,
reverse mode against an exact forward-mode tangent in rationals (in total and row by row), the numpy form in the documented order
against the exact form within the header's bound, the segment rule, the tangent's definition in mpmath (rows sum to 0; a central
difference of the exact x^e / sum in e), the host chain of d_e_dest for "A_drive", the header under a strict C compiler, and the
entries without a device."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from conftest import ROOT
import expected_reference as R
import expected_grad_reference as G
import expected_grad_dest_reference as D

ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_set_p_dest_tangent", "cpm_build_p_dest_tangent", "cpm_get_p_dest_tangent", "cpm_expected_grad_dest_dev", "cpm_expected_grad_dest",
       "cpm_expected_trip_tangent_dev", "cpm_expected_trip_tangent"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_grad_dest.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_GRAD_DEST_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.FLOWS_SYMBOLS, _lib.FLOWS_CSR_SYMBOLS, _lib.STAYS_SYMBOLS, _lib.PATHS_SYMBOLS,
                  _lib.CHARGE_SYMBOLS, _lib.OBJECTIVES_SYMBOLS, _lib.EXPECTED_SYMBOLS, _lib.EXPECTED_TRAVEL_SYMBOLS, _lib.EXPECTED_GRAD_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_grad_dest.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_expected_grad_dest.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_GRAD_DEST_H"]   # no new option, info key or flag
    assert '#include "cpm_expected_grad.h"' in text
    for method in ("set_p_dest_tangent", "build_p_dest_tangent", "get_p_dest_tangent", "expected_grad_dest", "expected_grad_dest_dev",
                   "expected_trip_tangent"):
        assert getattr(cpm.Sampler, method)


def test_segment_rule_is_the_one_of_the_p_drive_adjoint():
    """w is summed over the segments of a: the ordered product of the numpy form covers every destination exactly once, at the sizes
    tests/test_expected_grad.py lists"""
    for Z in list(range(1, 600)) + [1023, 1024, 1031, 2047, 2048, 2357, 4096, 8192, 20000]:
        n, seg_len = G.segments(Z)
        assert 1 <= n <= 64 and n * seg_len >= Z and (n - 1) * seg_len < Z, Z
        assert n == 1 or seg_len >= 32, Z
        assert -(-seg_len // 4) + 3 + n - 1 + 1 <= G.K(Z) // 2, Z       # the roundings behind a term of w are fewer than R
    for Z in (1, 2, 5, 33, 67, 129):
        M, mu = np.ones((Z, Z)), np.arange(1.0, Z + 1)                  # small integers: exact in any order
        assert np.array_equal(D._ordered_product(M, mu, Z), np.full(Z, Z * (Z + 1) / 2.0))


def _small_case(O, Z, T, seed):
    """tables with a zero row, a row with total below 1, a clipped p_drive entry, and a tangent whose rows do not sum to 0"""
    p_drive, p_dest = O.synth_p_drive(Z, T, 11), O.synth_p_dest_dense(Z, T, 11)
    p_dest[Z - 1, :, (T - 1) // 2] = 0.0                               # a zero row
    p_dest[0, :, :] *= 0.7                                             # a residual: it must not enter w
    p_drive[1 % Z, 0] = 1.5                                            # clipped
    dP = D.signed_tangent(p_dest, seed)
    tables = R.row_tables(p_dest)
    assert (tables[0] == 0.0).any() and (tables[2] > 0.25).any() and abs(dP[0].sum(axis=0)).min() > 0
    return p_drive, p_dest, dP, tables


@pytest.mark.parametrize("with_next", [False, True])
@pytest.mark.parametrize("flags", [0, R.IVP])
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("Z", [2, 3, 5])
def test_reverse_mode_equals_forward_mode_exactly_in_rationals(O, Z, T, flags, with_next):
    """sum(grad_dest) is the directional derivative of L along dP, and grad_dest[o, t] the derivative along dP masked to row (o, t),
    without rounding"""
    p_drive, p_dest, dP, tables = _small_case(O, Z, T, 100 * Z + T)
    pi0 = np.random.default_rng(3).uniform(0.0, 2.0, Z)
    gp, gd, gn = G.signed_cotangents(Z, T, 5)
    gn = gn if with_next else None
    gdest, _, grad, gpi0 = D.exact_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables)
    egrad, epi0 = G.exact_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables)
    assert np.array_equal(grad, egrad) and gpi0 == epi0                # the p_drive adjoint is untouched by the w terms

    def functional(dpark, ddrv, dnext):
        v = sum(Fraction(float(gp[o, t])) * dpark[o, t] + Fraction(float(gd[o, t])) * ddrv[o, t] for o in range(Z) for t in range(T))
        return v if gn is None else v + sum(Fraction(float(gn[o])) * dnext[o] for o in range(Z))

    assert functional(*D.exact_tangent_dest(p_drive, p_dest, dP, pi0, flags, tables)) == sum(gdest.ravel(), Fraction(0))
    for o in range(Z):
        for t in range(T):
            masked = np.zeros_like(dP)
            masked[o, :, t] = dP[o, :, t]
            assert functional(*D.exact_tangent_dest(p_drive, p_dest, masked, pi0, flags, tables)) == gdest[o, t], (o, t)
    zero_t = (T - 1) // 2
    assert gdest[Z - 1, zero_t] == 0                                   # the zero row carries no tangent


@pytest.mark.parametrize("flags", [0, R.IVP])
@pytest.mark.parametrize("Z,T", [(5, 3), (24, 24), (33, 2), (67, 24)])
def test_numpy_form_meets_the_bound_against_the_exact_form(O, Z, T, flags):
    p_drive, p_dest = R.modified_tables(O, Z, T)
    p_drive[:min(Z, 5), 1 % T] = [np.nan, -0.1, 0.0, 1.0, 1.5][:min(Z, 5)]
    tables = R.row_tables(p_dest)
    dP = D.signed_tangent(p_dest, Z + T)
    for kind, with_next in (("random", True), ("single", False)):
        gp, gd, gn = G.signed_cotangents(Z, T, Z + T, kind)
        gn = gn if with_next else None
        got, grad, gpi0 = D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, None, flags, gn, tables)
        exact, bound, egrad, epi0 = D.exact_adjoint_dest(p_drive, p_dest, dP, gp, gd, None, flags, gn, tables)
        w, z = G.worst_ratio(got, exact, bound)
        print(f"Z={Z} T={T} flags={flags} {kind}: grad_dest worst error / bound {w:.4f}")
        assert z and w <= 1.0
        bg, bp = G.bounds(p_drive, flags, *G.magnitudes(p_drive, p_dest, gp, gd, None, flags, gn, tables))
        assert G.worst_ratio(grad, egrad, bg)[0] <= 1.0 and G.worst_ratio(gpi0, epi0, bp)[0] <= 1.0
        fb = D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, None, flags, gn, tables, bound_factor=1.0)[0]   # the f64 form of the bound
        assert np.allclose(fb, np.array(bound, dtype=np.float64), rtol=1e-9, atol=0.0)
    zero = D.numpy_adjoint_dest(p_drive, p_dest, np.zeros_like(dP), gp, gd, None, flags, gn, tables)[0]
    assert not zero.any()


def _dest_rows(O, Z, T, density):
    dm, _ = O.synth_datamatrix(Z, T, 11, density=density)
    return D.e_dest_x(dm)


@pytest.mark.parametrize("e", [2, 0.5, 1.7])
def test_tangent_definition_rows_sum_to_zero_and_match_a_central_difference(O, e):
    """p * (ln x - sum p ln x) at the f64 p nearest to the exact x^e / sum x^e: the rows sum to 0 within what rounding p to f64 allows,
    and the tangent is the derivative of the exact law in e (Richardson: 4 |FD(h) - FD(h / 2)|)"""
    Z, T = 7, 3
    x = _dest_rows(O, Z, T, 0.6)
    mp = mpmath.mpf
    rows = 0
    for o in range(Z):
        for t in range(T):
            xr = x[o, :, t]
            if not (xr > 0).any():
                continue
            rows += 1
            p_exact = D.p_of_e_mp(xr, e)
            p64 = np.array([float(v) for v in p_exact])
            dP, bound = D.tangent_mp(xr, p64)
            n = int((p64 > 0).sum())
            lmax = max(abs(mpmath.log(mp(float(v)))) for v in xr if v > 0)
            assert abs(mpmath.fsum(dP)) <= 4 * n * mp(R.EPS) * (1 + lmax)       # sum p = 1 up to n roundings of p to f64
            fd = lambda h: [(a - b) / (2 * h) for a, b in zip(D.p_of_e_mp(xr, mp(e) + h), D.p_of_e_mp(xr, mp(e) - h))]
            f1, f2 = fd(mp(2) ** -10), fd(mp(2) ** -11)
            for d in range(Z):
                assert abs(dP[d] - f2[d]) <= 4 * abs(f1[d] - f2[d]), (o, t, d)
                assert p64[d] > 0.0 or dP[d] == 0
    assert rows > Z


def test_a_drive_chain_on_a_hand_made_case():
    from carparkingmaps_amd import model_selection as ms
    Z, T = 3, 2
    grad_dest = np.array([[0.5, -0.25], [0.125, 0.0], [-1.0, 2.0]])
    driving = np.array([[0.25, 0.5], [0.0, 0.125], [1.0, 0.75]])
    dw_sec = np.array([[7200.0, -3600.0], [100.0, 14400.0], [0.0, 7200.0]])
    assert ms.e_dest_param_grad(grad_dest) == 1.375
    direct = (0.25 * 7200 - 0.5 * 3600 + 0.125 * 14400 + 0.75 * 7200) / (T * 3600.0)
    assert ms.e_dest_param_grad(grad_dest, driving, dw_sec) == 1.375 + direct == 2.375
    # the scale is a_drive_grad's: A_drive = sum(driving * w_sec) / (T * 3600) is linear in w_sec
    w_sec = np.random.default_rng(1).uniform(100, 3000, (Z, T))
    a = lambda w: ms.expected_objectives(driving, driving, seconds=driving * w)["A_drive"]
    assert abs((a(w_sec + dw_sec) - a(w_sec)) - ms.e_dest_param_grad(np.zeros((Z, T)), driving, dw_sec)) < 1e-12
    assert np.array_equal(ms.a_drive_grad(dw_sec) * driving, driving * dw_sec / (T * 3600.0))


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_grad_dest_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_grad_dest.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[4] = {0};
    int32_t r[7];
    int i;
    r[0] = cpm_set_p_dest_tangent(ctx, a);
    r[1] = cpm_build_p_dest_tangent(ctx, NULL);
    r[2] = cpm_get_p_dest_tangent(ctx, a);
    r[3] = cpm_expected_grad_dest_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL, a, NULL, a);
    r[4] = cpm_expected_grad_dest(ctx, NULL, 0u, a, a, NULL, a, NULL, a);
    r[5] = cpm_expected_trip_tangent_dev(ctx, a);
    r[6] = cpm_expected_trip_tangent(ctx, a, a);
    for (i = 1; i < 7; ++i) if (r[i] != r[0]) return 1;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_grad_dest_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.run([exe]).returncode == (0 if _no_device(_lib.load()) else 2)


def test_every_entry_returns_err_hip_without_a_device(cpm):
    from carparkingmaps_amd import _lib
    L = _lib.load()
    a = np.zeros(8)
    vp = a.ctypes.data_as(ctypes.c_void_p)
    want = ERR_HIP if _no_device(L) else ERR_ARG
    assert L.cpm_set_p_dest_tangent(None, vp) == want
    assert L.cpm_build_p_dest_tangent(None, None) == want
    assert L.cpm_get_p_dest_tangent(None, vp) == want
    for flags in (0, _lib.CPM_EXPECT_IVP):
        assert L.cpm_expected_grad_dest_dev(None, None, flags, vp, None, vp, None, vp) == want
        assert L.cpm_expected_grad_dest(None, None, flags, vp, vp, None, vp, None, vp) == want
    assert L.cpm_expected_trip_tangent_dev(None, vp) == want
    assert L.cpm_expected_trip_tangent(None, vp, vp) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()
