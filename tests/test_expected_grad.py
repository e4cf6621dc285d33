"""The adjoint of the expected densities (include/cpm_expected_grad.h), without a GPU: the ABI list, reverse mode against forward mode
exactly in rationals, the numpy form against the exact form within the bound the device is held to, the host cotangents of the three
objectives and the chain rule to (p_min, p_max, e_drive) against central differences, the header under a strict C compiler, and the
entries without a device."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import expected_reference as R
import expected_grad_reference as G

ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_expected_grad_dev", "cpm_expected_grad"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


def test_grad_header_declares_exactly_the_two_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_grad.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_GRAD_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.FLOWS_SYMBOLS, _lib.FLOWS_CSR_SYMBOLS, _lib.STAYS_SYMBOLS, _lib.PATHS_SYMBOLS,
                  _lib.CHARGE_SYMBOLS, _lib.OBJECTIVES_SYMBOLS, _lib.EXPECTED_SYMBOLS, _lib.EXPECTED_TRAVEL_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_grad.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_expected_grad.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_GRAD_H"]   # no new option, info key or flag
    # the two headers it builds on declare what they declared
    assert _declared("cpm_expected.h") == sorted(_lib.EXPECTED_SYMBOLS) and len(_lib.EXPECTED_SYMBOLS) == 4
    assert _declared("cpm_expected_travel.h") == sorted(_lib.EXPECTED_TRAVEL_SYMBOLS) and len(_lib.EXPECTED_TRAVEL_SYMBOLS) == 6
    assert cpm.Sampler.expected_grad and cpm.Sampler.expected_grad_dev


def test_the_order_of_the_sums_keeps_K_under_the_cap():
    """K = twice the roundings behind a term must not exceed Z + 32 (include/cpm_expected_grad.h); the segments cover the row"""
    for Z in list(range(1, 600)) + [1023, 1024, 1031, 2047, 2048, 2357, 4096, 8192, 20000]:
        n, seg_len = G.segments(Z)
        assert 1 <= n <= 64 and n * seg_len >= Z and (n - 1) * seg_len < Z, Z      # no empty segment
        assert n == 1 or seg_len >= 32, Z
        assert G.K(Z) <= Z + 32, Z


def _directions(Z, T, seed, n):
    rng = np.random.default_rng(seed)
    return [rng.integers(-8, 9, (Z, T)).astype(np.float64) / 8.0 for _ in range(n)]


@pytest.mark.parametrize("flags", [0, R.IVP])
def test_reverse_mode_equals_forward_mode_exactly_in_rationals(O, flags):
    """<G, d out> in the direction (d pi_0, d p_drive) is <grad_pi0, d pi_0> + <grad_p_drive, d p_drive>, without rounding: every unit
    direction of pi_0 and 20 random directions of p_drive, on tables with a zero row, a D1 row and a row that ends in zeros."""
    Z, T = 5, 3
    p_drive, p_dest = R.modified_tables(O, Z, T)
    p_dest[3, :, 1] = 0.0                                  # (modified_tables places its rows at Z > 7 only: the same three kinds here)
    p_dest[1, :, :] *= 0.7
    p_dest[2, Z - 3:, :] = 0.0
    p_drive[0, 1], p_drive[4, 2], p_drive[2, 0] = 1.5, np.nan, 0.0   # clipped entries: the tangent does not follow them
    tables = R.row_tables(p_dest)
    assert (tables[0] == 0.0).any() and (tables[1][tables[0] != 0.0] != Z - 1).any() and (tables[2] > 0.25).any()
    pi0 = np.random.default_rng(3).uniform(0.0, 2.0, Z)
    gp, gd, gn = G.signed_cotangents(Z, T, 5)
    grad, gpi0 = G.exact_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables)
    assert all(grad[o, t] == 0 for o, t in ((0, 1), (4, 2), (2, 0)))

    def functional(dpark, ddrv, dnext):
        return (sum(Fraction(float(gp[o, t])) * dpark[o, t] + Fraction(float(gd[o, t])) * ddrv[o, t] for o in range(Z) for t in range(T))
                + sum(Fraction(float(gn[o])) * dnext[o] for o in range(Z)))

    zero_q = np.zeros((Z, T))
    for z in range(Z):
        e = np.zeros(Z)
        e[z] = 1.0
        assert functional(*G.exact_tangent(p_drive, p_dest, pi0, flags, e, zero_q, tables)) == gpi0[z], z
    for k, dq in enumerate(_directions(Z, T, 7, 20)):
        want = sum(grad[o, t] * Fraction(float(dq[o, t])) for o in range(Z) for t in range(T))
        assert functional(*G.exact_tangent(p_drive, p_dest, pi0, flags, np.zeros(Z), dq, tables)) == want, k
    # the exact forward states are those of the densities' own exact form
    epark, _, _ = R.exact_expected(p_drive, p_dest, pi0, flags, tables)
    states, _ = G._forward(p_drive, p_dest, pi0, flags, tables)
    pre, _ = R.schedule(T, flags)
    assert all(Fraction(states[pre + t][0][o], 1 << states[pre + t][1]) == epark[o, t] for o in range(Z) for t in range(T))


@pytest.mark.parametrize("flags", [0, R.IVP])
@pytest.mark.parametrize("Z,T", [(5, 3), (24, 24), (67, 24)])
def test_numpy_form_meets_the_bound_against_the_exact_form(O, Z, T, flags):
    """The bound of the header, relative to the magnitude recurrence, shown to be attainable by an f64 evaluation in another order of
    sums before the device is held to it; a word whose magnitude is 0 is 0."""
    p_drive, p_dest = R.modified_tables(O, Z, T)
    p_drive[:min(Z, 5), 1 % T] = [np.nan, -0.1, 0.0, 1.0, 1.5][:min(Z, 5)]
    tables = R.row_tables(p_dest)
    for kind, with_next in (("random", True), ("single", False)):
        gp, gd, gn = G.signed_cotangents(Z, T, Z + T, kind)
        gn = gn if with_next else None
        grad, gpi0 = G.numpy_adjoint(p_drive, p_dest, gp, gd, None, flags, gn, tables)
        egrad, epi0 = G.exact_adjoint(p_drive, p_dest, gp, gd, None, flags, gn, tables)
        bg, bp = G.bounds(p_drive, flags, *G.magnitudes(p_drive, p_dest, gp, gd, None, flags, gn, tables))
        wg, zg = G.worst_ratio(grad, egrad, bg)
        wp, zp = G.worst_ratio(gpi0, epi0, bp)
        print(f"Z={Z} T={T} flags={flags} {kind}: worst error / bound: grad_p_drive {wg:.4f}, grad_pi0 {wp:.4f}")
        assert zg and zp
        assert wg <= 1.0 and wp <= 1.0
        assert np.all(grad[~G.inside(p_drive)] == 0.0)
    grad, gpi0 = G.numpy_adjoint(p_drive, p_dest, *G.signed_cotangents(Z, T, 1, "zero")[:2], None, flags, None, tables)
    assert not grad.any() and not gpi0.any()


def _fd_check(f, x, grad, h, what):
    """every component of grad against central differences of f at steps h and h / 2: accepted when |grad - FD(h/2)| <= 4 |FD(h) -
    FD(h/2)| + 2^-30 max|grad| -- the yardstick is the finite difference's own truncation error"""
    x = np.array(x, dtype=np.float64)
    flat, g = x.reshape(-1), np.asarray(grad, dtype=np.float64).reshape(-1)
    floor = 2.0 ** -30 * np.abs(g).max()

    def fd(i, step):
        keep = flat[i]
        flat[i] = keep + step
        up = f(x)
        flat[i] = keep - step
        dn = f(x)
        flat[i] = keep
        return (up - dn) / (2 * step)

    worst = 0.0
    for i in range(flat.size):
        a, b = fd(i, h), fd(i, h / 2)
        tol = 4 * abs(a - b) + floor
        worst = max(worst, abs(g[i] - b) / tol)
        assert abs(g[i] - b) <= tol, (what, i, g[i], a, b)
    print(f"{what}: worst |grad - FD(h/2)| / tolerance {worst:.3f}")


def test_host_cotangents_against_central_differences():
    from carparkingmaps_amd import model_selection as ms
    Z, T = 7, 24
    rng = np.random.default_rng(17)
    drv, park = rng.uniform(0.01, 0.05, (Z, T)), rng.uniform(0.05, 0.25, (Z, T))     # random: no ties
    m_act, m_park = rng.uniform(0, 1, T), rng.uniform(0, 1, (Z, T))
    m_park[3] = 0.0                                       # an unmeasured zone
    park[5] = park[5, 0]                                  # a flat zone
    _fd_check(lambda d: ms.traffic_activity_error(ms.traffic_activity(d), m_act), drv, ms.traffic_activity_error_grad(drv, m_act), 2.0 ** -12,
              "activity_error")
    g = ms.parking_density_error_grad(park, m_park)
    assert not g[3].any() and not g[5].any()              # zones that are not valid give 0
    valid = [z for z in range(Z) if z not in (3, 5)]
    sub = lambda p: ms.parking_density_error(np.vstack([p[z] if z in valid else park[z] for z in range(Z)]), 1, m_park)
    _fd_check(sub, park, g, 2.0 ** -12, "parking_error")
    w_sec = rng.uniform(100, 3000, (Z, T))
    _fd_check(lambda d: ms.expected_objectives(park, d, seconds=d * w_sec)["A_drive"], drv, ms.a_drive_grad(w_sec), 2.0 ** -12, "A_drive")
    # the argmin and argmax terms are there: the gradient of a min-max normalised error sums to 0 over an hour-sum shift ...
    ga = ms.traffic_activity_error_grad(drv, m_act)
    assert abs(ga[0].sum()) <= 1e-12 * np.abs(ga[0]).sum() and np.array_equal(ga[0], ga[Z - 1])


def test_chain_rule_to_the_three_parameters_on_a_hand_made_table():
    from carparkingmaps_amd import model_selection as ms
    p_min, p_max, e = 0.15, 0.8, 0.6
    s = np.array([[0.0, 1.0, np.nan, 0.3, 0.7],
                  [0.5, 0.25, 0.9, 0.0, 1.0],
                  [2.0, 2.5, 3.0, 2.2, 4.0]])             # (the last row's p_drive is >= 1: clipped everywhere)
    with np.errstate(invalid="ignore"):
        table = lambda a, b, c: a + (b - a) * np.power(s, c)
        pd = table(p_min, p_max, e)
    on = G.inside(pd)
    assert not on[2].any() and not on[0, 2] and on[0, 0] and on[0, 1]     # p_min and p_max themselves are inside (0, 1)
    g = np.where(on, np.random.default_rng(2).uniform(-1, 1, s.shape), 0.0)  # as the library returns it: 0 where q is flat
    got = ms.p_drive_param_grads(g, s, p_min, p_max, e)
    assert all(np.isfinite(got))
    f = lambda x: float(np.sum(g[on] * table(x[0], x[1], x[2])[on]))
    _fd_check(f, [p_min, p_max, e], got, 2.0 ** -10, "chain rule")
    # by hand: the entries s = 0 and s = 1 carry no e_drive term, s = 0 no p_max term, s = 1 no p_min term
    only = np.zeros(s.shape)
    only[0, 0] = 2.0
    assert ms.p_drive_param_grads(only, s, p_min, p_max, e) == (2.0, 0.0, 0.0)
    only[0, 0], only[0, 1] = 0.0, 3.0
    assert ms.p_drive_param_grads(only, s, p_min, p_max, e) == (0.0, 3.0, 0.0)


def test_grad_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_grad_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_grad.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[4] = {0};
    int32_t r1 = cpm_expected_grad_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL, a, NULL);
    int32_t r2 = cpm_expected_grad(ctx, NULL, 0u, a, a, NULL, a, NULL);
    if (r1 != r2) return 1;
    return r1 == CPM_ERR_HIP ? 0 : r1 == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_grad_header")
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
        assert L.cpm_expected_grad_dev(None, None, flags, vp, None, vp, None) == want
        assert L.cpm_expected_grad(None, None, flags, vp, vp, None, vp, None) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()
