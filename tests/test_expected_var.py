"""Exact variances of a resample's counts (include/cpm_expected_var.h), without a GPU: the ABI list, the header under a strict C
compiler, the Python refusals, the numpy form of the definition within the header's bound of the exact (rational) form, exact
identities in rationals, and the condition of the statistical test on the CPU sampler alone: the mean over the cells of
(N - mean)^2 / var is 1 within 5.5 standard errors with the exact variance and is not with the binomial one."""
import ctypes
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import expected_reference as R
import expected_var_reference as V

T = 24
ERR_ARG, ERR_HIP = -1, -2


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_declares_exactly_the_two_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpm_expected_var.h")).read()
    declared = sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(["cpm_expected_var_dev", "cpm_expected_var"]) == sorted(_lib.EXPECTED_VAR_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.EXPECTED_SYMBOLS, _lib.EXPECTED_SPARSE_SYMBOLS, _lib.EXPECTED_TANGENT_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_var.h but not exported"
    assert not re.findall(r"#define (CPM_(?:OPT|INFO|EXPECT_)\w+)", text)       # no new option, info key or flag
    assert cpm.Sampler.expected_var and cpm.Sampler.expected_var_dev and cpm.Sampler.expected_var_words
    from carparkingmaps_amd import model_selection as ms
    assert ms.count_zscores


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_var_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_var.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[4] = {0};
    int32_t r1 = cpm_expected_var_dev(ctx, NULL, CPM_EXPECT_IVP, a), r2 = cpm_expected_var(ctx, a, 0u, a, NULL, a, NULL);
    if (r1 != r2) return 1;
    return r1 == CPM_ERR_HIP ? 0 : r1 == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_var_header")
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
        assert L.cpm_expected_var_dev(None, None, flags, vp) == want
        assert L.cpm_expected_var(None, vp, flags, vp, vp, vp, vp) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()


def test_count_zscores_refusals_and_fixed_cells():
    from carparkingmaps_amd import model_selection as ms
    ev = {"mean_parking": np.array([[2.0, 3.0]]), "var_parking": np.array([[0.0, 4.0]]),
          "mean_driving": np.array([[1.0, 1.0]]), "var_driving": np.array([[0.25, 0.0]])}
    z = ms.count_zscores(np.array([[2, 7]]), np.array([[2, 1]]), ev)
    assert np.isnan(z["parking"][0, 0]) and z["parking"][0, 1] == 2.0 and z["driving"][0, 0] == 2.0 and np.isnan(z["driving"][0, 1])
    assert z["parking_fixed"].tolist() == [[True, False]] and z["driving_fixed"].tolist() == [[False, True]]
    assert z["parking_fixed_ok"] and z["driving_fixed_ok"]
    assert not ms.count_zscores(np.array([[3, 7]]), np.array([[2, 1]]), ev)["parking_fixed_ok"]
    with pytest.raises(ValueError):
        ms.count_zscores(np.zeros((2, 2)), np.array([[2, 1]]), ev)                               # a shape
    with pytest.raises(ValueError):
        ms.count_zscores(np.array([[2, 7]]), np.array([[2, 1]]), dict(ev, var_parking=np.array([[-1.0, 4.0]])))
    with pytest.raises(ValueError):
        ms.count_zscores(np.array([[2, 7]]), np.array([[2, 1]]), dict(ev, var_driving=np.array([[np.nan, 0.0]])))


def test_python_refuses_a_start_of_the_wrong_shape(cpm):
    """the shape is refused in front of the library: no context is needed to see it (none can exist without a device)"""
    class Fake:
        Z, T = 4, 3
    with pytest.raises(ValueError):
        cpm.Sampler.expected_var(Fake(), start=np.ones(5))
    with pytest.raises(ValueError):
        cpm.Sampler.expected_var(Fake(), start=np.ones((4, 1)))


# ------------------------------------------------------------------------------------------------ the forms against each other
@functools.lru_cache(maxsize=None)
def _exact(O, Z, flags, weighted):
    p_drive, p_dest = R.modified_tables(O, Z, T)
    tables = R.row_tables(p_dest)
    w = None
    if weighted:                                      # (integers with a zero whose sum is a power of two: w / sum w is dyadic)
        w = np.random.default_rng(Z).integers(0, 50, Z).astype(np.float64)
        w[1] = 0.0
        w[0] += 2.0 ** np.ceil(np.log2(w.sum())) - w.sum()
    return p_drive, p_dest, tables, w, V.exact_var(p_drive, p_dest, w, flags, tables)


@pytest.mark.parametrize("flags", [0, V.IVP])
@pytest.mark.parametrize("Z", [2, 3, 8, 16, 17, 33])
def test_numpy_form_meets_the_bound_against_the_exact_form(O, Z, flags):
    """Shown here to be attainable by an f64 evaluation in another order of sums before the device is held to it."""
    p_drive, p_dest, tables, w, exact = _exact(O, Z, flags, Z % 2 == 1)
    got = V.numpy_var(p_drive, p_dest, w, flags, tables)
    worst, zeros_ok = V.worst(got, exact, Z, T, flags)
    print(f"Z={Z} flags={flags}: worst error / bound {worst}")
    assert zeros_ok, "a word whose exact value is 0 is not 0"
    assert max(worst.values()) <= 1.0


def test_integer_form_is_the_exact_form_on_dyadic_tables():
    for Z in (2, 3, 17):
        p_drive, p_dest, w = V.dyadic_tables(Z, 3)
        a, b = V.int_var(p_drive, p_dest, w), V.exact_var(p_drive, p_dest, w)
        n = V.numpy_var(p_drive, p_dest, w)
        for k in V.KEYS:
            assert (a[k] == b[k]).all(), k
            f, exact = V.to_f64(a[k])
            assert exact, "the dyadic tables are meant to be exact in f64"
            assert np.array_equal(f, n[k]), k              # (and so any correct f64 evaluation gives these bits)
        last, ell, r = R.row_tables(p_dest)
        assert (last == 0).any() and ((last > 0) & (last < 1)).any() and (w == 0).any()
        assert any(p_dest[o, o, t] > 0 for o in range(Z) for t in range(3))
        assert (p_drive < 0).any() and (p_drive > 1).any()


# ------------------------------------------------------------------------------------------------ identities in rationals
@pytest.mark.parametrize("flags", [0, V.IVP])
@pytest.mark.parametrize("Z", [3, 8, 17])
def test_exact_identities(O, Z, flags):
    p_drive, p_dest, tables, w, ex = _exact(O, Z, flags, True)
    C = Fraction(int(w.sum()))
    for s in (0, Z - 1):                                        # all cars in one zone: the count is binomial, the bound is attained
        e = np.zeros(Z)
        e[s] = 1.0
        one = V.exact_var(p_drive, p_dest, e, flags, tables)
        assert all(one["var_parking"][z, t] == one["mean_parking"][z, t] * (1 - one["mean_parking"][z, t]) for z in range(Z) for t in range(T))
    # the mean is (sum w) * pi_t of the exact expected reference with pi_0 = w / sum w
    pi0 = [Fraction(int(v)) / C for v in w]
    epark, edrv, _ = R.exact_expected(p_drive, p_dest, pi0, flags, tables)
    for t in range(T):
        for z in range(Z):
            assert ex["mean_parking"][z, t] == C * epark[z, t] and ex["mean_driving"][z, t] == C * edrv[z, t]
            pi, pd = epark[z, t], edrv[z, t]
            assert 0 <= ex["var_parking"][z, t] <= C * pi * (1 - pi) and 0 <= ex["var_driving"][z, t] <= C * pd * (1 - pd)
    if not flags:
        assert all(ex["var_parking"][z, 0] == 0 for z in range(Z))                       # hour 0 without the IVP: no spread at all
        assert any(ex["var_parking"][z, 1] > 0 for z in range(Z))


@pytest.mark.parametrize("flags", [0, V.IVP])
@pytest.mark.parametrize("Z", [3, 8, 17])
def test_every_row_of_the_transition_matrix_sums_to_one(Z, flags):
    """On tables in multiples of 2^-8 the row totals and r are exact, so the identity holds in rationals: with all cars in zone s the
    means over the zones add up to 1 in every hour.  (On other tables the f64 row total stands in the definition, as in
    cpm_expected.h, and the sum is 1 only within the bound.)"""
    p_drive, p_dest = V.dyadic8_tables(Z, T)
    last = R.row_tables(p_dest)[0]
    assert (last == 0).any() and ((last > 0) & (last < 1)).any()
    for s in (0, Z // 2, Z - 1):
        e = np.zeros(Z)
        e[s] = 1.0
        one = V.int_var(p_drive, p_dest, e, flags)
        assert all(sum(one["mean_parking"][:, t]) == 1 for t in range(T))
        if s == 0:
            other = V.exact_var(p_drive, p_dest, e, flags)
            assert all((one[k] == other[k]).all() for k in V.KEYS)


# ------------------------------------------------------------------------------------------------ the statistical condition
def test_statistic_on_the_cpu_sampler_and_the_binomial_mutant(O):
    p_drive, p_dest, zone0, w = V.stat_setup(O)
    C = len(zone0)
    cdf = O.build_cdf(p_dest)
    ev = V.numpy_var(p_drive, p_dest, w)
    runs = []
    for seed in range(1, V.RUNS + 1):
        r = O.fast_run(p_drive, cdf, C, seed, zone0, do_ivp=False)
        runs.append((r["parking"], r["driving"]))
    V.check_statistic(runs, ev, C, "cpu")


def test_statistic_with_the_ivp_on_the_cpu_sampler(O):
    """solve_ivp then resample from the same seed's two step ranges, against ivp=True"""
    p_drive, p_dest, zone0, w = V.stat_setup(O)
    C = len(zone0)
    cdf = O.build_cdf(p_dest)
    ev = V.numpy_var(p_drive, p_dest, w, V.IVP)
    runs = []
    for seed in range(1, V.RUNS + 1):
        r = O.fast_run(p_drive, cdf, C, seed, zone0, do_ivp=True)
        runs.append((r["parking"], r["driving"]))
    mean = np.stack([ev["mean_parking"], ev["mean_driving"]])
    var = np.stack([ev["var_parking"], ev["var_driving"]])
    g, kept = V.g_with(runs, mean, var, var)
    ok, m, half = V.within_cap(g, kept, list(range(T)))
    print(f"cpu ivp: all hours: exact {m:.4f} +- {half:.4f}")
    assert ok
    for t in range(0, 7):
        ok, m, half = V.within_cap(g, kept, [t])
        assert ok, f"hour {t}: {m:.4f} +- {half:.4f}"
