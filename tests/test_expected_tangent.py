"""Forward tangent of the expected densities (include/cpm_expected_tangent.h), without a GPU: the ABI list, the header under a strict C
compiler, the entries without a device, the numpy restatement of the header (tests/expected_tangent_reference.py) against the exact
(rational) tangent within the header's bound, the exact tangent against central differences of the exact densities, the transposition
identity <G, J v> = <J^T G, v> between the exact tangent and the exact adjoints as an EQUALITY of Fractions, the host's residual
derivatives against central differences, refine_expected_lm on a numpy evaluator, and what the host refuses before it touches the sampler."""
import ctypes
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

import expected_reference as R
import expected_grad_reference as G
import expected_grad_dest_reference as D
import expected_tangent_reference as TG
from test_expected_gpu import _pi0, _tables

ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_expected_tangent_dev", "cpm_expected_tangent", "cpm_build_p_drive_tangent_dev", "cpm_build_p_drive_tangent"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_tangent.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_TANGENT_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "EXPECTED_TANGENT_SYMBOLS"]
    assert len(others) >= 14
    for other in others:
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_tangent.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_expected_tangent.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_TANGENT_H", "CPM_TANGENT_MAX_DIRECTIONS"]   # no option, info key, status or flag
    assert "CPM_EXPECT_" not in "".join(re.findall(r"#define (\w+)", text)) and "0x100" not in code
    assert int(re.search(r"#define CPM_TANGENT_MAX_DIRECTIONS (\d+)", text).group(1)) == _lib.CPM_TANGENT_MAX_DIRECTIONS == 16
    assert '#include "cpm_expected_grad_dest.h"' in text
    for method in ("expected_tangent", "expected_tangent_dev", "build_p_drive_tangent", "build_p_drive_tangent_dev"):
        assert getattr(cpm.Sampler, method)


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_tangent_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_tangent.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[CPM_TANGENT_MAX_DIRECTIONS] = {0};
    int32_t r[4];
    int i;
    r[0] = cpm_expected_tangent_dev(ctx, 1, NULL, CPM_EXPECT_IVP, NULL, a, a, a, NULL, NULL);
    r[1] = cpm_expected_tangent(ctx, 1, NULL, 0u, a, a, NULL, a, a, NULL, NULL, NULL);
    r[2] = cpm_build_p_drive_tangent_dev(ctx, 0.1, 0.9, 0.5, a);
    r[3] = cpm_build_p_drive_tangent(ctx, 0.1, 0.9, 0.5, a);
    for (i = 1; i < 4; ++i) if (r[i] != r[0]) return 1;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_tangent_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
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
        assert L.cpm_expected_tangent_dev(None, 1, None, flags, None, vp, vp, vp, None, None) == want
        assert L.cpm_expected_tangent(None, 1, None, flags, vp, vp, vp, vp, vp, None, None, None) == want
    assert L.cpm_build_p_drive_tangent_dev(None, 0.1, 0.9, 0.5, vp) == want
    assert L.cpm_build_p_drive_tangent(None, 0.1, 0.9, 0.5, vp) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()


# ------------------------------------------------------------------ the references against each other
def _case(Z, Tc, seed):
    """(tables, K = 3 directions (pure p_drive | pure pi_0 | both), c_dest, a signed dP with zero rows left unplanted)"""
    p_drive, p_dest, tables = _tables(Z, Tc)
    d_pi0, d_pd = TG.directions(Z, Tc, 3, seed, p_drive)
    return p_drive, p_dest, tables, d_pi0, d_pd, np.array([0.0, -0.75, 1.5]), D.signed_tangent(p_dest, seed + 1)


@pytest.mark.parametrize("flags", [0, R.IVP])
@pytest.mark.parametrize("Z", [5, 12])
def test_numpy_tangent_meets_the_bound_against_the_exact_tangent(Z, flags):
    Tc = 3
    p_drive, p_dest, tables, d_pi0, d_pd, c, dP = _case(Z, Tc, 100 + Z)
    for kind in ("uniform", "given"):
        pi0 = _pi0(Z, kind)
        for k in range(3):
            args = (p_drive, p_dest, pi0, flags, d_pi0[:, k], d_pd[:, :, k], c[k], dP, tables)
            exact = TG.exact_direction(*args)
            bound = TG.exact_bounds(Z, Tc, flags, TG.magnitude(*args))
            got = TG.numpy_tangent(*args)
            for name, g, e, b in zip(("d parking", "d driving", "d pi_next"), got, exact, bound):
                w, z = TG.worst_ratio(g, e, b)
                print(f"Z={Z} flags={flags} pi0={kind} k={k} {name}: worst error / bound {w:.4f}")
                assert z and w <= 1.0
            # the magnitude dominates the exact tangent, word for word
            for e, m in zip(exact, TG.magnitude(*args)):
                assert all(abs(Fraction(a)) <= Fraction(b) for a, b in zip(np.asarray(e, dtype=object).ravel(), np.asarray(m, dtype=object).ravel()))


def _dyadic_case(Z, Tc, seed):
    """tables and directions on a coarse dyadic grid: p +- h * direction is exact in f64 for h = 2^-12, 2^-13, so a central
    difference of the exact densities differs from the derivative by its truncation alone"""
    p_drive, p_dest, _ = _tables(Z, Tc)
    q = lambda a, bits: np.round(np.asarray(a) * 2.0 ** bits) / 2.0 ** bits
    p_drive = np.asfortranarray(np.where(np.isnan(p_drive), np.nan, q(np.nan_to_num(p_drive), 20)))
    p_dest = np.asfortranarray(q(0.9 * p_dest, 20))
    rng = np.random.default_rng(seed)
    d_pi0 = q(rng.uniform(-1, 1, Z), 8)
    d_pd = np.asfortranarray(np.where(G.inside(p_drive), q(rng.uniform(-1, 1, (Z, Tc)), 8), 0.0))
    dP = np.asfortranarray(q(rng.uniform(-1, 1, p_dest.shape), 8))
    return p_drive, p_dest, R.row_tables(p_dest), d_pi0, d_pd, dP


@pytest.mark.parametrize("flags", [0, R.IVP])
def test_exact_tangent_matches_central_differences_of_the_exact_densities(flags):
    Z, Tc, c = 5, 3, 0.5
    p_drive, p_dest, tables, d_pi0, d_pd, dP = _dyadic_case(Z, Tc, 7)
    zero = tables[0] == 0.0
    dPm = dP.copy()
    for t, o in np.argwhere(zero):
        dPm[o, :, t] = 0.0                      # (a zero row stays one: the definition moves no entry of it)
    pi0 = np.round(_pi0(Z, "given") * 2.0 ** 20) / 2.0 ** 20
    tan = TG.exact_direction(p_drive, p_dest, pi0, flags, d_pi0, d_pd, c, dP, tables)
    fd = []
    for h in (2.0 ** -12, 2.0 ** -13):
        side = []
        for sg in (1.0, -1.0):
            pd = np.where(G.inside(p_drive), np.nan_to_num(p_drive) + sg * h * d_pd, p_drive)
            side.append(R.exact_expected(np.asfortranarray(pd), np.asfortranarray(p_dest + sg * h * c * dPm), pi0 + sg * h * d_pi0, flags, tables))
        hf = Fraction(h)
        fd.append([(np.asarray(u, dtype=object) - np.asarray(d, dtype=object)) / (2 * hf) for u, d in zip(*side)])
    checked = 0
    for t_arr, coarse, fine in zip(tan, fd[0], fd[1]):
        for a, d1, d2 in zip(np.asarray(t_arr, dtype=object).ravel(), coarse.ravel(), fine.ravel()):
            assert abs(Fraction(a) - d2) <= abs(d1 - d2), (float(a), float(d1), float(d2))
            checked += d1 != d2
    assert checked >= Z                          # (the map is not linear: the differences do have a truncation error)


@pytest.mark.parametrize("flags", [0, R.IVP])
@pytest.mark.parametrize("Z", [5, 12])
def test_transposition_identity_holds_exactly_between_the_exact_tangent_and_the_exact_adjoints(Z, flags):
    """<G, J v> + <g_next, d pi_next> == <grad_p_drive, dq> + <grad_pi0, d pi_0> + c * sum(grad_dest), as Fractions"""
    Tc = 3
    p_drive, p_dest, tables, d_pi0, d_pd, c, dP = _case(Z, Tc, 200 + Z)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 300 + Z)
    F = lambda a: np.array([Fraction(float(v)) for v in np.asarray(a).ravel()], dtype=object)
    for kind in ("uniform", "given"):
        pi0 = _pi0(Z, kind)
        grad_dest, _, grad_pd, grad_pi0 = D.exact_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables)
        plain_pd, plain_pi0 = G.exact_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables)
        assert (grad_pd == plain_pd).all() and list(grad_pi0) == list(plain_pi0)
        for k in range(3):
            dpark, ddrv, dnext = TG.exact_direction(p_drive, p_dest, pi0, flags, d_pi0[:, k], d_pd[:, :, k], c[k], dP, tables)
            lhs = (F(gp) * dpark.ravel()).sum() + (F(gd) * ddrv.ravel()).sum() + (F(gn) * np.array(dnext, dtype=object)).sum()
            dq = np.where(G.inside(p_drive), d_pd[:, :, k], 0.0)
            rhs = (grad_pd.ravel() * F(dq)).sum() + (np.array(grad_pi0, dtype=object) * F(d_pi0[:, k])).sum() + Fraction(float(c[k])) * grad_dest.sum()
            assert lhs == rhs and (k == 1 or lhs != 0), (Z, flags, kind, k, float(lhs), float(rhs))


# ------------------------------------------------------------------ the host's residual derivatives
def _fd(f, x, dx):
    """(derivative of f along dx by central differences at the finer of two steps, its error judged by the gap between the two)"""
    ds = [(f(x + h * dx) - f(x - h * dx)) / (2 * h) for h in (1e-5, 5e-6)]
    return ds[1], np.abs(ds[0] - ds[1]) + 1e-9 * np.abs(ds[1]) + 1e-10


@pytest.mark.parametrize("Z,T", [(5, 24), (12, 6)])
def test_residual_jvps_match_central_differences(cpm, Z, T):
    from carparkingmaps_amd import model_selection as ms
    rng = np.random.default_rng(40 + Z)
    p = rng.random((Z, T)) / Z
    x = p * rng.random((Z, T))
    m_p, m_a = rng.random((Z, T)), rng.random(T)
    m_p[2] = 0.0                                                     # an unmeasured zone
    p[1] = p[1, 0]                                                   # a flat zone
    dp, dx = rng.standard_normal((3, Z, T)) / Z, rng.standard_normal((3, Z, T)) / Z
    dp[:, 1] = 0.0                                                   # (it stays flat)
    w_sec, dw = 300.0 + 900.0 * rng.random((Z, T)), rng.standard_normal((Z, T))
    r, Jr = ms.activity_residual_jvp(x, dx, m_a)
    assert abs((r * r).sum() - ms.traffic_activity_error(ms.traffic_activity(x), m_a)) <= 1e-14
    rp, Jp = ms.parking_residual_jvp(p, dp, m_p)
    assert abs((rp * rp).sum() - ms.parking_density_error(p, 1, m_p)) <= 1e-14
    assert not rp[1].any() and not rp[2].any() and not Jp[:, 1].any() and not Jp[:, 2].any()
    ja = ms.a_drive_jvp(w_sec, dx)
    jd = ms.a_drive_jvp(w_sec, dx, x, dw)
    assert (ja[:2] == jd[:2]).all() and abs(jd[2] - ja[2] - (x * dw).sum() / (T * 3600.0)) <= 1e-12 * abs(jd[2])
    for k in range(3):
        want, err = _fd(lambda v: ms.activity_residual_jvp(v, dx, m_a)[0], x, dx[k])
        assert (np.abs(Jr[k] - want) <= err).all()
        want, err = _fd(lambda v: ms.parking_residual_jvp(v, dp, m_p)[0], p, dp[k])
        assert (np.abs(Jp[k] - want) <= err).all()
        want, err = _fd(lambda v: (v * w_sec).sum() / (T * 3600.0), x, dx[k])
        assert abs(ja[k] - want) <= err
    # the gradient of the mean squared errors, 2 J^T r, is the reverse-mode cotangent contracted with the direction
    g_act, g_park = ms.traffic_activity_error_grad(x, m_a), ms.parking_density_error_grad(p, m_p)
    for k in range(3):
        assert abs(2 * (Jr[k] * r).sum() - (g_act * dx[k]).sum()) <= 1e-12 * np.abs(g_act * dx[k]).sum()
        assert abs(2 * (Jp[k] * rp).sum() - (g_park * dp[k]).sum()) <= 1e-12 * np.abs(g_park * dp[k]).sum()
    flat = np.full((Z, T), 0.25)
    r, Jr = ms.activity_residual_jvp(flat, dx, m_a)
    assert np.isnan(r).all() and not Jr.any()


# ------------------------------------------------------------------ Levenberg-Marquardt on a numpy evaluator
def lm_run(ms, evaluator, jacobian, **kw):
    start = ms.Point(*TG.LM_START, TG.LM_E_DEST)
    return ms.refine_expected_lm(evaluator, [start], TG.LM_WEIGHTS, steps=TG.LM_STEPS, jacobian=jacobian, **kw)[0]


def lm_check(out, ratio, lo, hi, min_gap):
    Fs = [f for _, f in out["path"]]
    assert all(b < a for a, b in zip(Fs, Fs[1:])), Fs                      # non-increasing: only a decrease is accepted
    for pt, _ in out["path"]:
        x = np.array([pt.e_drive, pt.p_min, pt.p_max])
        assert (x >= lo).all() and (x <= hi).all() and pt.p_min + min_gap <= pt.p_max + 1e-15
    print(f"refine_expected_lm: F {Fs[0]:.6e} -> {Fs[-1]:.6e} (ratio {Fs[-1] / Fs[0]:.3e}) in {out['calls']} Jacobian calls, lam {out['lam']:.3e}")
    assert Fs[-1] <= ratio * Fs[0]
    assert out["calls"] <= TG.LM_STEPS + 1 and out["lam"] > 0 and len(out["gradient"]) == 3 and out["result"]["F"] == Fs[-1]


LM_CPU_RATIO = 3.2e-15   # F(last) / F(start) of the numpy run below; the tests hold a run to 10 times this


def test_refine_expected_lm_descends_the_planted_problem_on_a_numpy_evaluator(cpm):
    """The planted problem (expected_tangent_reference.lm_problem): Z = 12, T = 6, activity and parking measured at LM_TRUE, so F = 0
    there; from LM_START the numpy run reaches F = 1.334e-16 from 4.181e-02 in LM_STEPS = 4 steps, every one accepted: the ratio
    3.19e-15 that LM_CPU_RATIO records.  Both this run and the device's (tests/test_expected_tangent_gpu.py) must reach 10 times that
    ratio: the factor absorbs the device's different rounding.  (Four steps, not more: two steps later F is at the rounding floor of
    the densities, 5e-32, which says nothing about the method.)"""
    from carparkingmaps_amd import model_selection as ms
    from oracle import oracle as O
    O.build()
    ev, jac = TG.numpy_evaluator(TG.lm_problem(O))
    out = lm_run(ms, ev, jac)
    lm_check(out, 10 * LM_CPU_RATIO, np.array([1e-3, 0.0, 0.0]), np.array([16.0, 1.0, 1.0]), 1e-3)
    # bounds that bind: the path stays inside them
    box = {"e_drive": (1.0, 2.0), "p_min": (0.0, 0.1), "p_max": (0.8, 1.0)}
    out = lm_run(ms, ev, jac, bounds=box, min_gap=0.75)
    lm_check(out, 1.0, np.array([1.0, 0.0, 0.8]), np.array([2.0, 0.1, 1.0]), 0.75)


# ------------------------------------------------------------------ refusals before the sampler is touched
class _Untouchable:
    """a sampler that fails the test on any use"""
    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched: {name}")


def test_refine_expected_lm_refuses_before_it_touches_the_sampler(cpm):
    from carparkingmaps_amd import model_selection as ms
    ev = ms.Evaluator(_Untouchable(), C=1, seed=1, measured_activity=np.zeros(24), measured_parking=None)
    same = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(0.6, 0.2, 0.8, 2)]
    mixed = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(0.5, 0.1, 0.9, 1.5)]
    call = lambda pts, weights=None, **kw: ms.refine_expected_lm(ev, pts, weights, **kw)
    with pytest.raises(ValueError, match="share e_dest"):
        call(mixed, {"activity_error": 1.0})
    with pytest.raises(ValueError, match="unknown weight keys"):
        call(same, {"a_drive": 1.0})
    with pytest.raises(ValueError, match="measured_parking"):
        call(same, {"parking_error": 1.0})
    with pytest.raises(ValueError, match="weight dicts"):
        call(same, [{"activity_error": 1.0}])
    with pytest.raises(ValueError, match="negative weight"):
        call(same, {"activity_error": -1.0})
    with pytest.raises(ValueError, match="bounds that cross"):
        call(same, {"activity_error": 1.0}, bounds={"p_min": (0.5, 0.2)})
    with pytest.raises(ValueError, match="bounds that cross"):
        call(same, {"activity_error": 1.0}, bounds={"p_min": (0.9, 1.0), "p_max": (0.0, 0.5)})
    with pytest.raises(ValueError, match="unknown bound"):
        call(same, {"activity_error": 1.0}, bounds={"e_dest": (1.0, 2.0)})
    with pytest.raises(ValueError, match="lam0"):
        call(same, {"activity_error": 1.0}, lam0=0.0)
    ev2 = ms.Evaluator(_Untouchable(), C=1, seed=1, measured_activity=None, measured_parking=np.ones((3, 24)))
    with pytest.raises(ValueError, match="measured_activity"):
        ms.refine_expected_lm(ev2, same)
