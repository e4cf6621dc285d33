"""Expected parking and driving densities by Markov propagation (include/cpm_expected.h), without a GPU: the ABI list, the numpy form
of the definition against the exact (rational) form within the bound the device is held to, the definition against the CPU sampler
on tables with a zero row, a D1 row and a row that ends in zeros, mass, the host objectives, the header under a strict C compiler,
and the entries without a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import expected_reference as R

T = 24
SEED = 20240611
CAP = 5.5  # the cap of tests/test_oracle.py::test_sampled_density_matches_markov_propagation
ERR_ARG, ERR_HIP = -1, -2


def _declared():
    text = open(os.path.join(ROOT, "include", "cpm_expected.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


def test_expected_header_declares_exactly_the_four_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared()
    assert declared == sorted(["cpm_expected_dev", "cpm_expected_batch_dev", "cpm_expected", "cpm_expected_batch"]) == sorted(_lib.EXPECTED_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.FLOWS_SYMBOLS, _lib.FLOWS_CSR_SYMBOLS, _lib.STAYS_SYMBOLS, _lib.PATHS_SYMBOLS,
                  _lib.CHARGE_SYMBOLS, _lib.OBJECTIVES_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_expected.h")).read()
    assert {k: int(v) for k, v in re.findall(r"#define (CPM_\w+) (\d+)u", text)} == {"CPM_EXPECT_IVP": _lib.CPM_EXPECT_IVP}
    assert not re.findall(r"#define (CPM_(?:OPT|INFO)\w+)", text)         # no new option or info key
    assert cpm.Sampler.expected and cpm.Sampler.expected_batch and cpm.Sampler.expected_dev and cpm.Sampler.expected_batch_dev
    assert cpm.Sampler.expected_words


@pytest.mark.parametrize("flags", [0, R.IVP])
@pytest.mark.parametrize("Z", [5, 24, 67])
def test_numpy_form_meets_the_bound_against_the_exact_form(O, Z, flags):
    """h operators cost a word at most h * (Z + 7) roundings of non-negative terms; the bound is twice that.  Shown here to be
    attainable by an f64 evaluation in another order of sums before the device is held to it."""
    p_drive, p_dest = R.modified_tables(O, Z, T)
    tables = R.row_tables(p_dest)
    park, drv, nxt = R.numpy_expected(p_drive, p_dest, None, flags, tables)
    epark, edrv, enxt = R.exact_expected(p_drive, p_dest, None, flags, tables)
    h = np.array(R.operators_behind(T, flags))
    worst_p, zeros_p = R.worst_ratio(park, epark, np.array([R.bound(Z, k) for k in h])[None, :])
    worst_d, zeros_d = R.worst_ratio(drv, edrv, np.array([R.bound_driving(Z, k) for k in h])[None, :])
    worst_n, zeros_n = R.worst_ratio(nxt, enxt, R.bound(Z, h[-1] + 1))
    print(f"Z={Z} flags={flags}: worst error / bound: parking {worst_p:.3f}, driving {worst_d:.3f}, pi_next {worst_n:.3f}")
    assert zeros_p and zeros_d and zeros_n
    assert worst_p <= 1.0 and worst_d <= 1.0 and worst_n <= 1.0
    if not flags:
        assert all(epark[z, 0] == R.Fraction(1.0 / Z) for z in range(Z))


def _zscores(counts, driving, park, drv, C):
    dens = counts / C
    sigma = np.sqrt(park * (1 - park) / C)
    zp = np.abs(dens - park) / np.maximum(sigma, 1e-12)
    sd = np.sqrt(C * drv * (1 - drv))
    zd = np.abs(driving - C * drv) / np.maximum(sd, 1e-12)
    return zp, zd


@pytest.mark.parametrize("ivp", [False, True])
@pytest.mark.parametrize("Z,cpz", [(24, 4000), (67, 2000)])
def test_definition_is_the_law_of_the_cpu_sampler_and_the_textbook_form_is_not(O, Z, cpz, ivp):
    """The sampler does not renormalise a row, and a draw above a row total below 1 goes to the row's last zone with p > 0 (D1): the
    sampled densities lie within the 5.5 sigma cap of the definition and far outside it of markov_expected_density."""
    C = Z * cpz
    p_drive, p_dest = R.modified_tables(O, Z, T)
    r = O.fast_run(p_drive, O.build_cdf(p_dest), C, SEED, np.arange(C) // cpz + 1, do_ivp=ivp)
    park, drv, _ = R.numpy_expected(p_drive, p_dest, None, R.IVP if ivp else 0)
    zp, zd = _zscores(r["parking"], r["driving"], park, drv, C)
    print(f"Z={Z} ivp={ivp}: parking {zp.max():.2f} sigma, driving {zd.max():.2f} sigma")
    assert zp.max() < CAP and zd.max() < CAP
    if not ivp:
        assert np.array_equal(r["parking"][:, 0] / C, park[:, 0])      # hour 0 is exact
        pis = O.markov_expected_density(p_drive, p_dest, np.full(Z, 1.0 / Z)).T
        zt = np.abs(r["parking"] / C - pis) / np.maximum(np.sqrt(pis * (1 - pis) / C), 1e-12)
        print(f"  markov_expected_density: {zt.max():.1f} sigma")
        assert zt.max() > CAP                                           # the D1 rows are observed


@pytest.mark.parametrize("Z", [5, 24, 67])
def test_mass_stays_within_the_bound(O, Z):
    p_drive, p_dest = R.modified_tables(O, Z, T)
    pi0 = np.random.default_rng(Z).uniform(0.0, 2.0, Z)
    for flags in (0, R.IVP):
        park, _, nxt = R.numpy_expected(p_drive, p_dest, pi0, flags)
        m0 = math.fsum(pi0)
        h = R.operators_behind(T, flags)
        for t in range(T):
            assert abs(math.fsum(park[:, t]) - m0) <= R.bound(Z, h[t]) * m0, (flags, t)
        assert abs(math.fsum(nxt) - m0) <= R.bound(Z, h[-1] + 1) * m0


def test_row_total_above_one_is_refused_by_the_references(O):
    p_drive, p_dest = R.modified_tables(O, 24, T)
    p_dest[2, :, 4] *= 1.25
    with pytest.raises(R.TableError) as e:
        R.row_tables(p_dest)
    assert (e.value.hour, e.value.origin) == (5, 3)


def test_expected_objectives_go_through_the_existing_functions(O):
    from carparkingmaps_amd import model_selection as ms
    Z, C = 24, 4096                                   # (a power of two: C * pi / C is pi bit for bit)
    p_drive, p_dest = R.modified_tables(O, Z, T)
    park, drv, _ = R.numpy_expected(p_drive, p_dest)
    rng = np.random.default_rng(5)
    m_act, m_park = rng.uniform(0, 1, T), rng.uniform(0, 1, (Z, T))
    m_park[3] = 0.0                                   # an unmeasured zone
    out = ms.expected_objectives(park, drv, m_act, m_park)
    assert set(out) == {"traffic_activity", "activity_error", "parking_error"}          # no A_drive
    assert np.array_equal(out["traffic_activity"], ms.traffic_activity(drv))
    assert out["activity_error"] == ms.traffic_activity_error(ms.traffic_activity(drv), m_act)
    assert out["parking_error"] == ms.parking_density_error(C * park, C, m_park)
    assert set(ms.expected_objectives(park, drv)) == {"traffic_activity"}
    assert set(ms.expected_objectives(park, drv, measured_parking=m_park)) == {"traffic_activity", "parking_error"}


def test_expected_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[4] = {0};
    int32_t r1 = cpm_expected_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL), r2 = cpm_expected_batch_dev(ctx, NULL, 0u, a);
    int32_t r3 = cpm_expected(ctx, NULL, 0u, a, a, NULL), r4 = cpm_expected_batch(ctx, a, CPM_EXPECT_IVP, a, a);
    if (r1 != r2 || r1 != r3 || r1 != r4) return 1;
    return r1 == CPM_ERR_HIP ? 0 : r1 == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.run([exe]).returncode == (0 if _no_device(_lib.load()) else 2)


def test_every_entry_returns_err_hip_without_a_device(cpm):
    """No context can exist without a device, so the entries are called with none: CPM_ERR_HIP where no device is usable (with one,
    the null context is the argument error of every other entry)."""
    from carparkingmaps_amd import _lib
    L = _lib.load()
    a = np.zeros(8)
    vp = a.ctypes.data_as(ctypes.c_void_p)
    want = ERR_HIP if _no_device(L) else ERR_ARG
    for flags in (0, _lib.CPM_EXPECT_IVP):
        assert L.cpm_expected_dev(None, None, flags, vp, None) == want
        assert L.cpm_expected_batch_dev(None, vp, flags, vp) == want
        assert L.cpm_expected(None, None, flags, vp, vp, None) == want
        assert L.cpm_expected_batch(None, vp, flags, vp, vp) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()
