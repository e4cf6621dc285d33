"""The exact seed variance of travel seconds, kilometres and count functionals (include/cpm_expected_travel_var.h), without a GPU: the
ABI list, the header under a strict C compiler, the Python refusals; the exact recurrence against the enumeration of every path of
one car with the trip reward; identities in rationals; the numpy form in the documented order within the header's bound of the exact
form; v(a) of the documented f64 form against mpmath on the travel ladder; and the statistical test on the CPU sampler alone: over 400
seeds the mean of (L - mean)^2 / var is 1 within 5.5 standard errors, and is not for the two mutants."""
import ctypes
import functools
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import expected_reference as R
import expected_travel_reference as TR
import expected_var_reference as V
import expected_linear_var_reference as LV
import expected_travel_var_reference as TV
import travel_ladder as TL

T = 24
ERR_ARG, ERR_HIP = -1, -2
SYMS = ["cpm_expected_trip_var_dev", "cpm_expected_trip_var", "cpm_expected_trip_var_builds", "cpm_expected_travel_var_dev", "cpm_expected_travel_var"]


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_declares_exactly_the_five_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpm_expected_travel_var.h")).read()
    declared = sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(SYMS) == sorted(_lib.EXPECTED_TRAVEL_VAR_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.EXPECTED_SYMBOLS, _lib.EXPECTED_TRAVEL_SYMBOLS, _lib.EXPECTED_VAR_SYMBOLS, _lib.EXPECTED_LINEAR_VAR_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_travel_var.h but not exported"
    assert not re.findall(r"#define (CPM_(?:OPT|INFO|EXPECT_)\w+)", text)       # no new option, info key or flag
    assert cpm.Sampler.expected_travel_var and cpm.Sampler.expected_travel_var_dev and cpm.Sampler.expected_trip_var and cpm.Sampler.expected_trip_var_dev
    from carparkingmaps_amd import model_selection as ms
    assert ms.travel_noise and "travel" in ms.Evaluator.expected_noise.__code__.co_varnames


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_travel_var_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_travel_var.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[4] = {0};
    int32_t r1 = cpm_expected_travel_var_dev(ctx, NULL, CPM_EXPECT_IVP, 1, a, a, NULL);
    int32_t r2 = cpm_expected_travel_var(ctx, a, 0u, 1, a, a, NULL, NULL, a, a, NULL, NULL);
    int32_t r3 = cpm_expected_trip_var_dev(ctx, a), r4 = cpm_expected_trip_var(ctx, a);
    int64_t r5 = cpm_expected_trip_var_builds(ctx);
    if (r1 != r2 || r1 != r3 || r1 != r4 || r1 != r5) return 1;
    return r1 == CPM_ERR_HIP ? 0 : r1 == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_travel_var_header")
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
    for flags in (0, _lib.CPM_EXPECT_IVP):
        assert L.cpm_expected_travel_var_dev(None, None, flags, 1, vp, vp, vp) == want
        assert L.cpm_expected_travel_var(None, vp, flags, 1, vp, vp, vp, vp, vp, vp, vp, vp) == want
    assert L.cpm_expected_trip_var_dev(None, vp) == want and L.cpm_expected_trip_var(None, vp) == want
    assert L.cpm_expected_trip_var_builds(None) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()


def test_python_refuses_coefficients_and_a_start_of_the_wrong_shape(cpm):
    """the shapes are refused in front of the library: no context is needed to see it (none can exist without a device)"""
    class Fake:
        Z, T = 4, 3
    ok = np.zeros((4, 3))
    for a, b in ((np.zeros((4, 2)), np.zeros((4, 2))), (ok, np.zeros((4, 3, 1))), (np.zeros((3, 4)), np.zeros((3, 4))), (np.zeros(12), np.zeros(12)),
                 (np.zeros((4, 3, 0)), np.zeros((4, 3, 0))), (np.zeros((4, 3, 2, 1)), np.zeros((4, 3, 2, 1)))):
        with pytest.raises(ValueError):
            cpm.Sampler.expected_travel_var(Fake(), a, b)
    for bad in (np.zeros((4, 3, 1)), np.zeros((3, 4)), np.zeros(12)):
        with pytest.raises(ValueError):
            cpm.Sampler.expected_travel_var(Fake(), ok, ok, s_seconds=bad)
        with pytest.raises(ValueError):
            cpm.Sampler.expected_travel_var(Fake(), ok, ok, d_km=bad)
    with pytest.raises(ValueError):
        cpm.Sampler.expected_travel_var(Fake(), ok, ok, ok, ok, start=np.ones(5))


# ------------------------------------------------------------------------------------------------ every path of one car
def _tiny(Z, Tc):
    """tables in multiples of 2^-8 with a zero row, rows below 1, p_drive clipped at both ends; a datamatrix with standard deviations
    of every kind and a diagonal that is not 300 s / 1 km"""
    p_drive, p_dest = V.dyadic8_tables(Z, Tc)
    p_drive[0, 0], p_drive[Z - 1, Tc - 1] = 1.0, 0.0
    rng = np.random.default_rng(Z * 10 + Tc)
    dm = np.zeros((Z, Z, Tc, 2), order="F")
    dm[..., 0] = rng.uniform(300.0, 2400.0, (Z, Z, Tc))
    dm[..., 1] = dm[..., 0] * rng.choice([0.0, 0.05, 0.3, 2.0, -0.2], (Z, Z, Tc))
    dist = np.asfortranarray(rng.uniform(0.5, 30.0, (Z, Z)))
    return p_drive, p_dest, dm, dist


@pytest.mark.parametrize("flags", [0, TV.IVP])
@pytest.mark.parametrize("Tc", [3, 4])
@pytest.mark.parametrize("Z", [2, 3])
def test_exact_recurrence_is_the_enumeration_of_every_path(O, Z, Tc, flags):
    """an equality of Fractions, with the f64 words of var_sec as the variances of the draws"""
    p_drive, p_dest, dm, dist = _tiny(Z, Tc)
    tables = R.row_tables(p_dest)
    assert (tables[0] == 0).any() and ((tables[0] > 0) & (tables[0] < 1)).any()
    sec, km = TR.trip_values(dm, dist)
    vs = TV.var_sec_array(O, dm)
    assert (vs > 0).any() and (vs == 0).any()
    vsec = TV.vsec_exact(p_dest, [[[Fraction(float(vs[o, d, t])) for t in range(Tc)] for d in range(Z)] for o in range(Z)], tables)
    A, B, S, D = TV.signed_functionals(Z, Tc, 2, 10 * Z + Tc)
    w = np.arange(1, Z + 1).astype(np.float64)
    for k in range(2):
        f = [x[:, :, k] for x in (A, B, S, D)]
        mean, var = TV.brute_force(p_drive, p_dest, *f, sec, km, vs, w, flags, tables)
        fr = TV.fraction_tv(p_drive, p_dest, *f, sec, km, vsec, w, flags, tables)
        assert (fr["mean"], fr["var"]) == (mean, var) and var > 0
        it = TV.int_tv(p_drive, p_dest, *f, sec, km, vsec, w, flags, tables)
        assert all(it[key] == fr[key] for key in ("mean", "var", "zone_mean", "zone_var"))


# ------------------------------------------------------------------------------------------------ identities in rationals
@pytest.mark.parametrize("flags", [0, TV.IVP])
@pytest.mark.parametrize("Z", [3, 8])
def test_exact_identities(O, Z, flags):
    Tc = 6
    p_drive, p_dest, dm, dist = _tiny(Z, Tc)
    tables = R.row_tables(p_dest)
    sec, km = TR.trip_values(dm, dist)
    vsec = TV.vsec_numpy(p_dest, TV.var_sec_array(O, dm), tables)
    w = np.array([40.0, 16.0, 8.0] if Z == 3 else [20.0, 4.0, 8.0, 0.0, 16.0, 2.0, 6.0, 8.0])     # (64 cars: w / 64 is exact)
    A, B, S, D = TV.signed_functionals(Z, Tc, 1, Z)
    A, B, S, D = (x[:, :, 0] for x in (A, B, S, D))
    zero = np.zeros((Z, Tc))
    # S = D = 0: the linear reference's words
    lin = LV.int_lv(p_drive, p_dest, A, B, w, flags, tables)
    got = TV.int_tv(p_drive, p_dest, A, B, zero, zero, sec, km, vsec, w, flags, tables)
    assert all(got[k] == lin[k] for k in ("mean", "var", "zone_mean", "zone_var"))
    # S = 1: the mean is C x the exact expected seconds, D = 1: the kilometres
    park, drv, _ = R.exact_expected(p_drive, p_dest, w / w.sum(), flags, tables)
    ew_sec, ew_km = TR.exact_trip(p_dest, dm, dist, tables)
    _, _, tot_sec, tot_km = TR.exact_travel(drv, ew_sec, ew_km)
    one = np.ones((Z, Tc))
    sres = TV.int_tv(p_drive, p_dest, zero, zero, one, zero, sec, km, vsec, w, flags, tables)
    kres = TV.int_tv(p_drive, p_dest, zero, zero, zero, one, sec, km, vsec, w, flags, tables)
    assert sres["mean"] == int(w.sum()) * tot_sec and kres["mean"] == int(w.sum()) * tot_km
    assert sres["var"] > 0 and kres["var"] > 0
    # a functional constant over the zones with S = D = 0 still gives exactly 0
    c = np.asfortranarray(np.broadcast_to(np.arange(1.0, Tc + 1.0)[None, :] * 0.3, (Z, Tc)))
    const = TV.int_tv(p_drive, p_dest, c, zero, zero, zero, sec, km, vsec, w, flags, tables)
    assert const["var"] == 0 and all(v == 0 for v in const["zone_var"])


# ------------------------------------------------------------------------------------------------ the forms against each other
@functools.lru_cache(maxsize=None)
def _setup(O, Z, Tc):
    p_drive, p_dest = TR.planted_tables(O, Z, Tc) if Z > 2 else R.modified_tables(O, Z, Tc)
    dm, dist = TR.planted_datamatrix(O, Z, Tc)
    tables = R.row_tables(p_dest)
    sec, km = TR.trip_values(dm, dist)
    vsec = TV.vsec_numpy(p_dest, TV.var_sec_array(O, dm), tables)
    w = np.random.default_rng(Z).integers(0, 50, Z).astype(np.float64)
    w[1] = 0.0
    return p_drive, p_dest, tables, sec, km, vsec, w


@pytest.mark.parametrize("flags", [0, TV.IVP])
@pytest.mark.parametrize("Z", [2, 3, 8, 16, 17, 33])
def test_numpy_form_meets_the_bound_against_the_exact_form(O, Z, flags):
    """Shown here to be attainable by an f64 evaluation in the documented order before the device is held to it (both forms take the
    same v_sec words: the bound's B_v is slack here)"""
    Tc = 4
    p_drive, p_dest, tables, sec, km, vsec, w = _setup(O, Z, Tc)
    f = [x[:, :, 0] for x in TV.signed_functionals(Z, Tc, 1, 100 + Z)]
    ww = w if Z % 2 else None
    exact = TV.int_tv(p_drive, p_dest, *f, sec, km, vsec, ww, flags, tables)
    mag = TV.int_tv(p_drive, p_dest, *f, sec, km, vsec, ww, flags, tables, magnitude=True)
    got = TV.numpy_tv(p_drive, p_dest, *f, sec, km, vsec, ww, flags, tables)
    worst, zeros_ok = TV.worst(got, exact, TV.bounds(Z, Tc, flags, mag, ww))
    print(f"Z={Z} flags={flags}: worst error / bound {worst}")
    assert zeros_ok and max(worst.values()) <= 1.0
    assert exact["var"] > 0
    if Z <= 3:
        assert all(TV.fraction_tv(p_drive, p_dest, *f, sec, km, vsec, ww, flags, tables)[k] == exact[k] for k in ("mean", "var"))
    plain = TV.plain_tv(p_drive, p_dest, *f, sec, km, vsec, ww, flags, tables)
    assert abs(plain["var"] - got["var"]) <= 1e-9 * got["var"] and abs(plain["mean"] - got["mean"]) <= 1e-9 * float(mag["mean"])


def test_numpy_form_with_no_trip_coefficients_has_the_bits_of_the_linear_form(O):
    for Z in (17, 33):
        p_drive, p_dest, tables, sec, km, vsec, w = _setup(O, Z, 4)
        A, B = LV.signed_functionals(Z, 4, 1, Z)
        zero = np.zeros((Z, 4))
        for flags in (0, TV.IVP):
            a = LV.numpy_lv(p_drive, p_dest, A[:, :, 0], B[:, :, 0], w, flags, tables)
            b = TV.numpy_tv(p_drive, p_dest, A[:, :, 0], B[:, :, 0], zero, zero, sec, km, vsec, w, flags, tables)
            assert a["mean"] == b["mean"] and a["var"] == b["var"] and np.array_equal(a["zone_var"], b["zone_var"])


def test_integer_form_fits_f64_on_the_dyadic_tables_and_numpy_gives_its_bits():
    for Z in (2, 3, 17):
        p_drive, p_dest, w = V.dyadic_tables(Z, 3)
        dm, dist = TV.dyadic_datamatrix(Z, 3)
        sec, km = TR.trip_values(dm, dist)
        vsec = np.zeros((Z, 3))
        A, B, S, D = TV.small_functionals(Z, 3, 2, Z)
        for k in range(2):
            f = [x[:, :, k] for x in (A, B, S, D)]
            it = TV.int_tv(p_drive, p_dest, *f, sec, km, vsec, w, 0, bits=53)
            n = TV.numpy_tv(p_drive, p_dest, *f, sec, km, vsec, w, 0)
            assert float(it["mean"]) == n["mean"] and float(it["var"]) == n["var"]
            assert [float(x) for x in it["zone_var"]] == list(n["zone_var"]) and [float(x) for x in it["zone_mean"]] == list(n["zone_mean"])
            assert (it["var"] > 0 or Z < 17) and np.any(S[:, :, k] != 0)
    with pytest.raises(TV.NotExact):                        # (the assertion can fail: random means leave the 53 bits)
        p_drive, p_dest, dm, dist = _tiny(3, 3)
        sec, km = TR.trip_values(dm, dist)
        f = [x[:, :, 0] for x in TV.signed_functionals(3, 3, 1, 1)]
        TV.int_tv(p_drive, p_dest, *f, sec, km, np.zeros((3, 3)), None, 0, bits=53)


# ------------------------------------------------------------------------------------------------ v(a) against mpmath
def _ladder_cells():
    """(mean, std word) of every rung of tests/travel_ladder.py on three means, 'none' (0) included"""
    cells = []
    for mean in (62.72, 961.0, 2380.13):
        for rung in TL.RUNGS:
            cells.append((mean, math.inf if math.isinf(rung) else mean * rung))
    return cells


def test_v_of_the_documented_form_against_mpmath_on_the_travel_ladder(O):
    import mpmath as mp
    worst = 0.0
    for mean, sd in _ladder_cells():
        got, want = TV.var_sec_f64(O, mean, sd), TV.var_sec_mp(mean, sd)
        rung = sd / mean
        if rung < 0 or math.isinf(rung):                    # sigma <= 0, and a mass of 0: the draw is the mean
            assert got == 0.0 and want == 0
            continue
        assert want > 0 and got > 0
        err = float(abs(mp.mpf(got) - want) / want)
        worst = max(worst, err)
        assert err <= TV.V_BOUND + 2 * TV.EPS, (mean, sd, err / TV.V_BOUND)
    print(f"var_sec: worst relative error {worst:.3e} = {worst / TV.V_BOUND:.3f} of the bound")
    # both sides of the series' threshold, far below it (where 1 - 2 a phi / E would cancel) and far above it
    for a in [1e-8, 1e-4, 1e-2, 0.025, 0.1, 0.5, 0.999, 1.0, math.nextafter(1.0, 2.0), 1.001, 1.439, 2.0, 5.0, 8.47, 9.09, 38.0, 100.0, 1e5]:
        E = O.lib().orc_erf(a * TV.SQRT_HALF)
        got, want = TV.v_f64(O, a, E), TV.v_mp(a)
        assert abs(mp.mpf(got) - want) <= TV.V_BOUND * want, (a, float(abs(mp.mpf(got) - want) / want) / TV.V_BOUND)
    assert TV.v_f64(O, 1e-4, O.lib().orc_erf(1e-4 * TV.SQRT_HALF)) == pytest.approx(1e-8 / 3, rel=1e-8)
    for mean, sd in ((0.0, 0.0), (0.0, 5.0), (-3.0, 1.0), (100.0, -1.0), (100.0, math.inf), (0.0, math.inf)):
        assert TV.var_sec_f64(O, mean, sd) == 0.0 and TV.var_sec_mp(mean, sd) == 0


# ------------------------------------------------------------------------------------------------ the statistical condition
def _cpu_runs(O, p_drive, p_dest, zone0, dm, dist, ivp):
    cdf = O.build_cdf(p_dest)
    runs = []
    for seed in range(1, TV.RUNS + 1):
        r = O.fast_run(p_drive, cdf, len(zone0), seed, zone0, do_ivp=ivp, datamatrix=dm, dist=dist)
        runs.append((r["parking"], r["driving"], r["sum_tt_q16"] / 65536.0))
    return runs


def _cpu_stat(O, ivp):
    p_drive, p_dest, zone0, w, dm, dist = TV.stat_setup(O)
    flags = TV.IVP if ivp else 0
    tables = R.row_tables(p_dest)
    sec, km = TR.trip_values(dm, dist)
    vsec = TV.vsec_numpy(p_dest, TV.var_sec_array(O, dm), tables)
    funcs = TV.stat_functionals(TV.STAT_Z, TV.STAT_T)
    res = [TV.numpy_tv(p_drive, p_dest, *f[1:], sec, km, vsec, w, flags, tables) for f in funcs]
    mean, var = np.array([r["mean"] for r in res]), np.array([r["var"] for r in res])
    for k, f in enumerate(funcs):
        plain = TV.plain_tv(p_drive, p_dest, *f[1:], sec, km, vsec, w, flags, tables)
        assert abs(plain["var"] - var[k]) <= 1e-9 * var[k]
    L = TV.stat_values(_cpu_runs(O, p_drive, p_dest, zone0, dm, dist, ivp), funcs)
    return L, mean, var


def test_statistic_on_the_cpu_sampler(O):
    """the total seconds, and the total seconds plus a random signed count functional, on the tables of the linear call's test (on
    them both mutants lie inside the cap: the tests below plant tables for each)"""
    TV.check_stat(*_cpu_stat(O, False), "cpu")


def test_statistic_with_the_ivp_on_the_cpu_sampler(O):
    TV.check_stat(*_cpu_stat(O, True), "cpu ivp")


@pytest.mark.parametrize("ivp", [False, True])
def test_covariance_of_destination_and_duration_and_the_mutant_without_it(O, ivp):
    """p_drive = 1, no draw noise, seconds(o, d) = 600 (1 + h[o] + h[d]): the trip's seconds and the value of where it ends move
    together; the form that adds the two spreads separately is a factor of about 2 low"""
    p_drive, p_dest, zone0, w, dm, dist = TV.cov_setup(O)
    flags = TV.IVP if ivp else 0
    tables = R.row_tables(p_dest)
    sec, km = TR.trip_values(dm, dist)
    vsec = TV.vsec_numpy(p_dest, TV.var_sec_array(O, dm), tables)
    assert np.all(vsec == 0.0)
    Z, Tc = p_drive.shape
    zero, one = np.zeros((Z, Tc)), np.ones((Z, Tc))
    res = TV.numpy_tv(p_drive, p_dest, zero, zero, one, zero, sec, km, vsec, w, flags, tables)
    mut = TV.plain_tv(p_drive, p_dest, zero, zero, one, zero, sec, km, vsec, w, flags, tables, mutant="no_cov")
    assert 1.8 < res["var"] / mut["var"] < 2.1
    runs = _cpu_runs(O, p_drive, p_dest, zone0, dm, dist, ivp)
    L = np.array([[r[2]] for r in runs])
    TV.check_stat(L, np.array([res["mean"]]), np.array([res["var"]]), "cpu covariance", [("no_cov", 0, np.array([mut["var"]]))])


@pytest.mark.parametrize("ivp", [False, True])
def test_draw_noise_alone_and_the_mutant_without_it(O, ivp):
    """p_drive = 1, one destination per row, equal means: the path is fixed, ALL noise of the seconds is draw noise and
    var = C * T * sd^2 * v(a); the form without S^2 v_sec says 0"""
    p_drive, p_dest, zone0, w, dm, dist = TV.draw_only_setup(O)
    flags = TV.IVP if ivp else 0
    tables = R.row_tables(p_dest)
    sec, km = TR.trip_values(dm, dist)
    vsec = TV.vsec_numpy(p_dest, TV.var_sec_array(O, dm), tables)
    Z, Tc = p_drive.shape
    zero, one = np.zeros((Z, Tc)), np.ones((Z, Tc))
    res = TV.numpy_tv(p_drive, p_dest, zero, zero, one, zero, sec, km, vsec, w, flags, tables)
    C = len(zone0)
    closed = C * Tc * 100.0 ** 2 * float(TV.v_mp(1.0))
    assert abs(res["var"] - closed) <= 1e-12 * closed and res["mean"] == C * Tc * 1000.0
    mut = TV.plain_tv(p_drive, p_dest, zero, zero, one, zero, sec, km, vsec, w, flags, tables, mutant="no_draw")
    assert mut["var"] == 0.0
    runs = _cpu_runs(O, p_drive, p_dest, zone0, dm, dist, ivp)
    L = np.array([[r[2]] for r in runs])
    TV.check_stat(L, np.array([res["mean"]]), np.array([res["var"]]), "cpu draw noise", [("no_draw", 0, np.array([mut["var"]]))])
