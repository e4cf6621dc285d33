"""The seed variances from the compact rows (include/cpm_expected_sparse_var.h), without a GPU: one backward operator's three sums
restated in numpy in the order of the dense kernels, with every destination, zeros included, against the order of the sparse kernels
over the stored cells alone -- equal in every bit and in the sign of every zero -- for the count form and the travel form, at the sizes
the GPU test uploads; the exact 0 of a constant functional; two mutants that must differ; the two orders of the trip variance weight on
the travel ladder's standard deviations, with a passing and a failing case of the header's precondition; the header, the exports and
the refusals that need no device."""
import ctypes
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import expected_sparse_grad_reference as G
import expected_sparse_reference as S
import expected_sparse_var_reference as SV
import expected_travel_var_reference as TV
import travel_ladder as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 403, 518, 1031, 1089]
TC = 2
ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_expected_sparse_linear_var_dev", "cpm_expected_sparse_linear_var", "cpm_expected_sparse_trip_var_dev", "cpm_expected_sparse_trip_var",
       "cpm_expected_sparse_trip_var_builds", "cpm_expected_sparse_travel_var_dev", "cpm_expected_sparse_travel_var"]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(np.signbit(a), np.signbit(b))


@functools.lru_cache(maxsize=None)
def _case(Z):
    """the hand-made tables with kept cells of weight 0, a planted cancellation in hour 0, the states (hour TC - 1: all zeros), the
    coefficients and the trip values of one size: computed once, shared"""
    _, p_dest, info = S.sparse_tables(Z, TC)
    rng = np.random.default_rng(2000 + Z)
    mean = rng.uniform(-50.0, 3000.0, (Z, Z))
    dist = rng.uniform(0.1, 40.0, (Z, Z))
    sec, km = G.trip_values(mean, dist)
    Sc, Dc = rng.normal(0.0, 1.0, Z), rng.normal(0.0, 0.1, Z)
    Sc[::5] = 0.0
    Dc[1::5] = 0.0
    hours = []
    for t in range(TC):
        p_t = np.array(p_dest[:, :, t])
        mu, nu = SV.state(Z, t, zeros=t == TC - 1)
        if t == 0 and Z >= 6:
            SV.plant_cancellation(p_t, mu)
        keep = G.kept_zero_cells(p_t)
        hours.append((p_t, G.rows_of(p_t, keep), keep, mu, nu))
    return hours, (Sc, Dc, sec, km), info


# ------------------------------------------------------------------ the geometry and the cases
def test_segment_counts_are_pinned():
    got = {Z: (G.grad_segments(Z), G.segment_len(Z, G.grad_segments(Z))) for Z in SIZES}
    assert got == {2: (1, 2), 403: (12, 34), 518: (16, 33), 1031: (32, 33), 1089: (34, 33)}
    assert 1031 - 31 * 33 == 8 and 33 * 33 == 1089                                      # 8 destinations in the last segment; an EMPTY last segment
    assert [G.trip_segments(Z, 3) for Z in SIZES] == [1, 7, 8, 8, 8]
    assert G.grad_segments(358) == 11 and G.grad_segments(2357) == 54


def test_the_cases_hold_what_they_are_meant_to():
    hours, (Sc, Dc, sec, km), info = _case(403)
    p_t, rows, keep, mu, nu = hours[0]
    assert (mu < 0).any() and (mu > 0).any() and (mu == 0).any() and (nu == 0).any() and (nu >= 0).all()        # signed mu
    assert not hours[TC - 1][3].any() and not hours[TC - 1][4].any()                    # the hour whose state is all zeros
    assert all(not p_t[o].any() for o in info["zero"]) and len(info["zero"]) == 2       # zero rows
    totals = p_t.sum(axis=1)
    assert sum(0.4 < x < 0.6 for x in totals) >= 3 and (totals <= 1.0).all()            # rows below 1 (residual rows)
    assert len(keep) > 50 and all((d, 0.0) in rows[o] for o, d in keep)                 # kept cells of weight 0
    assert rows[2] == [(1, 0.25), (5, 0.25)]                                            # the planted row: terms that cancel exactly
    part = SV.sparse_sums(rows, mu, nu, 403)
    assert part[0, 0, 2] == 0.0 and not np.signbit(part[0, 0, 2]) and part[0, 1, 2] == 2 * 0.375 * 1.5     # s1 cancels exactly to +0, s2 does not
    assert (Sc == 0).any() and (Sc < 0).any() and (Dc == 0).any() and (sec < 0).any() and sec[7, 7] == 300.0 and km[7, 7] == 1.0
    assert all(r == sorted(r) and len({d for d, _ in r}) == len(r) for r in rows)


# ------------------------------------------------------------------ the two orders
@pytest.mark.parametrize("Z", SIZES)
def test_sparse_order_gives_the_bits_of_the_dense_order_for_the_counts(Z):
    hours, _, _ = _case(Z)
    nseg = G.grad_segments(Z)
    for t, (p_t, rows, _, mu, nu) in enumerate(hours):
        dense = SV.dense_sums(p_t, mu, nu)
        sparse = SV.sparse_sums(rows, mu, nu, Z)
        assert dense.shape == (nseg, 3, Z) and _bits_equal(dense, sparse), (Z, t)
        assert not np.signbit(dense[dense == 0.0]).any()                                # a chain never becomes -0
        assert _bits_equal(SV.finish(dense), SV.finish(sparse))
    first = SV.dense_sums(*[hours[0][k] for k in (0, 3, 4)])                            # (not a comparison of zeros; Z = 2: mu[1] is mu[0] and
    assert Z == 2 or all(first[:, k].any() for k in range(3))                           # nu[1] is 0, every term is 0)
    assert not SV.dense_sums(*[hours[TC - 1][k] for k in (0, 3, 4)]).any()              # the all-zero state: every word +0


@pytest.mark.parametrize("Z", SIZES)
def test_sparse_order_gives_the_bits_of_the_dense_order_for_travel(Z):
    hours, (Sc, Dc, sec, km), _ = _case(Z)
    assert np.isfinite(sec).all() and np.isfinite(km).all()                             # the precondition of the header
    e = SV.edge(Sc, Dc, sec, km)
    for t, (p_t, rows, _, mu, nu) in enumerate(hours):
        dense = SV.dense_sums(p_t, mu, nu, e)
        sparse = SV.sparse_sums(rows, mu, nu, Z, SV.edge_of(Sc, Dc, sec, km))
        assert _bits_equal(dense, sparse), (Z, t)
        assert dense[:, :2].any()                                                       # (zeta = e behind the zeroed state: still a product)
    zero = np.zeros(Z)                                                                  # S = D = 0: the words of the count form
    p_t, rows, _, mu, nu = hours[0]
    assert _bits_equal(SV.sparse_sums(rows, mu, nu, Z, SV.edge_of(zero, zero, sec, km)), SV.sparse_sums(rows, mu, nu, Z))


@pytest.mark.parametrize("c", [1.0, 1e6])
def test_a_constant_functional_gives_exactly_zero_in_the_sparse_order(c):
    for Z in (403, 1089):
        p_t, rows, _, _, nu = _case(Z)[0][0]
        mu = np.full(Z, c * 0.3)                                                        # (0.3 c is no power of two: p * mu rounds)
        part = SV.sparse_sums(rows, mu, nu, Z)
        assert not part[:, :2].any() and not np.signbit(part[:, :2]).any()
        assert _bits_equal(part, SV.dense_sums(p_t, mu, nu))


def test_mutants_differ():
    Z = 1031                                                                            # seg_len = 33: begin & 3 != 0 for most segments
    p_t, rows, _, mu, nu = _case(Z)[0][0]
    good = SV.sparse_sums(rows, mu, nu, Z)
    by_d = SV.sparse_sums(rows, mu, nu, Z, chain=lambda d, begin: d & 3)
    assert not _bits_equal(good, by_d)
    scale = np.abs(SV.finish(good)).max(axis=1, keepdims=True)
    assert (np.abs(SV.finish(by_d) - SV.finish(good)) <= 1e-12 * scale).all()           # (a mutant of the order, not of the value)
    raw = SV.uncentred_sums(rows, mu, nu, Z)
    assert not _bits_equal(raw[:2], SV.finish(good)[:2]) and _bits_equal(raw[2], SV.finish(good)[2])
    assert (np.abs(raw - SV.finish(good)) <= 1e-9 * np.maximum(scale, 1.0)).all()
    const = np.full(Z, 1e6)                                                             # the constant functional at c = 10^6
    raw = SV.uncentred_sums(rows, const, nu, Z)
    cv = raw[1] - raw[0] * raw[0]
    assert cv.any(), "the uncentred shortcut should leave a variance for the constant functional"
    centred = SV.finish(SV.sparse_sums(rows, const, nu, Z))
    assert not (centred[1] - centred[0] * centred[0]).any()


# ------------------------------------------------------------------ v_sec
@functools.lru_cache(maxsize=None)
def _ladder(Z):
    """one hour of the ladder's datamatrix (standard deviations from 4 x the mean to 0, negative and infinite) and its var_sec"""
    from oracle import oracle as O
    O.build()
    dm, _, idx = TL.ladder_datamatrix(O, Z, 3, 5, 0.5)
    dm, idx = np.asfortranarray(dm[:, :, :1]), idx[:, :, 0]
    assert Z < 65 or len(set(idx[idx >= 0].tolist())) == len(TL.RUNGS)                  # every rung is there
    return dm, TV.var_sec_array(O, dm)[:, :, 0]


@pytest.mark.parametrize("Z", [2, 65, 129, 403])
def test_trip_variance_weight_orders_agree_on_the_ladder(Z):
    _, var_sec = _ladder(Z)
    assert np.isfinite(var_sec).all() and (var_sec > 0).any() and (var_sec == 0).any()  # the precondition, and both exits
    _, p_dest, _ = S.sparse_tables(Z, TC)
    p_t = np.ascontiguousarray(p_dest[:, :, 0])
    rows = G.rows_of(p_t, G.kept_zero_cells(p_t))
    for T in (1, 3, 24):
        dense, sparse = SV.dense_vsec(p_t, var_sec, T), SV.sparse_vsec(rows, var_sec, Z, T)
        assert dense.shape == (G.trip_segments(Z, T), Z) and _bits_equal(dense, sparse), (Z, T)
    assert dense.any()


def test_precondition_on_cells_that_are_not_stored(O):
    """the header's rule, on the host restatement of etv_var_sec: var_sec is not finite exactly where a = (0.1 * mean) / sd is +inf
    or sd * v * sd overflows; a cell that is not stored must not hold such a pair"""
    f = lambda m, s: TV.var_sec_f64(O, m, s)
    assert np.isnan(f(np.inf, 5.0)) and np.isnan(f(1e300, 1e-300)) and f(1e200, 1e160) == np.inf            # the failing pairs
    for m, s in ((np.inf, 0.0), (np.inf, np.inf), (np.nan, 3.0), (np.nan, 0.0), (5.0, np.nan), (5.0, np.inf), (-np.inf, 2.0), (-3.0, 0.0),
                 (700.0, -1.0), (1e150, 0.0), (1e-300, 1e-300), (2.0 ** 510, 2.0 ** 510)):                 # pairs the rule lets pass
        assert np.isfinite(f(m, s)), (m, s)
    Z = 65
    _, var_sec = _ladder(Z)
    _, p_dest, _ = S.sparse_tables(Z, TC)
    p_t = np.ascontiguousarray(p_dest[:, :, 0])
    rows = G.rows_of(p_t)
    o, d = next((o, d) for o in range(3, Z) for d in range(Z) if p_t[o, d] == 0.0 and d != o and p_t[o].any())
    ok = np.array(var_sec)
    ok[o, d] = f(np.inf, 0.0)                                                           # passes: +inf mean, no std word -> a = NaN -> 0
    assert _bits_equal(SV.dense_vsec(p_t, ok, 3), SV.sparse_vsec(rows, ok, Z, 3))
    bad = np.array(var_sec)
    bad[o, d] = f(np.inf, 5.0)                                                          # fails: the dense order forms 0 * NaN
    with np.errstate(invalid="ignore"):
        dense = SV.dense_vsec(p_t, bad, 3)
    sparse = SV.sparse_vsec(rows, bad, Z, 3)
    assert np.isnan(dense[:, o]).any() and np.isfinite(sparse).all() and not _bits_equal(dense, sparse)
    assert _bits_equal(np.delete(dense, o, axis=1), np.delete(sparse, o, axis=1))       # (only that origin's word)


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
    declared = _declared("cpm_expected_sparse_var.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_SPARSE_VAR_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "EXPECTED_SPARSE_VAR_SYMBOLS"]
    assert len(others) >= 22
    for other in others:
        assert not set(declared) & set(other)
    L = _lib.load()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_sparse_var.h but not exported"
        want = ctypes.c_int64 if name.endswith("_builds") else ctypes.c_int32
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is want
    dense = {"cpm_expected_sparse_linear_var": "cpm_expected_linear_var", "cpm_expected_sparse_trip_var": "cpm_expected_trip_var",
             "cpm_expected_sparse_travel_var": "cpm_expected_travel_var"}
    for name in declared:                                                               # the argument lists of the namesakes
        twin = name.replace("_sparse", "")
        assert twin in _lib.EXPECTED_LINEAR_VAR_SYMBOLS + _lib.EXPECTED_TRAVEL_VAR_SYMBOLS and any(twin.startswith(v) for v in dense.values())
        assert list(getattr(L, name).argtypes) == list(getattr(L, twin).argtypes), name
    text = open(os.path.join(ROOT, "include", "cpm_expected_sparse_var.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_SPARSE_VAR_H"]      # no option, info key, status or flag of its own
    for h in os.listdir(os.path.join(ROOT, "include")):                                 # included from nowhere else
        if h != "cpm_expected_sparse_var.h":
            assert '#include "cpm_expected_sparse_var.h"' not in open(os.path.join(ROOT, "include", h)).read()
    for word in ("grad_segments", "(d - s * seg_len) & 3", "((c0 + c1) + c2) + c3", "1,089", "finite", "CPM_INFO_P_DENSE", "a == +inf", "2^511"):
        assert word in text, word                                                       # the derivation and the preconditions are stated
    for h in ("cpm_expected_linear_var.h", "cpm_expected_travel_var.h"):                # the dense headers point here
        assert "cpm_expected_sparse_var.h" in open(os.path.join(ROOT, "include", h)).read()
    for method in ("expected_linear_var", "expected_linear_var_dev", "expected_trip_var", "expected_trip_var_dev", "expected_trip_var_builds",
                   "expected_travel_var", "expected_travel_var_dev"):
        assert inspect.signature(getattr(cpm.Sampler, method)).parameters["sparse"].default is False, method
    from carparkingmaps_amd import model_selection as M
    for fn in (M.activity_noise, M.objective_noise, M.travel_noise):
        assert inspect.signature(fn).parameters["sparse"].default is False, fn.__name__
    src = inspect.getsource(M.Evaluator.expected_noise)
    assert src.count("sparse=sparse") == 4 and "sparse = self.expected_sparse" in src   # the three noises and expected()


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_sparse_var_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_sparse_var.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[8] = {0};
    int32_t r[6];
    int64_t n;
    int i;
    r[0] = cpm_expected_sparse_linear_var_dev(ctx, NULL, CPM_EXPECT_IVP, 1, a, a, NULL);
    r[1] = cpm_expected_sparse_linear_var(ctx, NULL, 0u, 1, a, a, a, a, NULL, NULL);
    r[2] = cpm_expected_sparse_trip_var_dev(ctx, a);
    r[3] = cpm_expected_sparse_trip_var(ctx, a);
    r[4] = cpm_expected_sparse_travel_var_dev(ctx, NULL, 0u, 1, a, a, NULL);
    r[5] = cpm_expected_sparse_travel_var(ctx, NULL, CPM_EXPECT_IVP, 1, a, a, NULL, NULL, a, a, NULL, NULL);
    n = cpm_expected_sparse_trip_var_builds(ctx);
    for (i = 1; i < 6; ++i) if (r[i] != r[0]) return 1;
    if (n != (int64_t)r[0]) return 1;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_sparse_var_header")
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
        assert L.cpm_expected_sparse_linear_var_dev(None, None, flags, 1, vp, vp, None) == want
        assert L.cpm_expected_sparse_linear_var(None, None, flags, 1, vp, vp, vp, vp, None, None) == want
        assert L.cpm_expected_sparse_travel_var_dev(None, None, flags, 1, vp, vp, None) == want
        assert L.cpm_expected_sparse_travel_var(None, None, flags, 1, vp, vp, None, None, vp, vp, None, None) == want
    assert L.cpm_expected_sparse_trip_var_dev(None, vp) == want
    assert L.cpm_expected_sparse_trip_var(None, vp) == want
    assert L.cpm_expected_sparse_trip_var_builds(None) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()
    assert not a.any()


class _NoDevice:
    """a Sampler whose library must not be reached: a wrong shape with sparse=True is refused before any device call"""
    Z, T = 4, 2

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came too late: {name} was touched")


def test_wrong_shapes_are_refused_before_any_device_call(cpm):
    ok, short, deep = np.zeros((4, 2)), np.zeros((4, 1)), np.zeros((4, 2, 0))
    for a, b in ((ok, short), (short, short), (deep, deep), (np.zeros(4), np.zeros(4))):
        with pytest.raises(ValueError, match="expected_linear_var"):
            cpm.Sampler.expected_linear_var(_NoDevice(), a, b, sparse=True)
        with pytest.raises(ValueError, match="expected_travel_var"):
            cpm.Sampler.expected_travel_var(_NoDevice(), a, b, sparse=True)
    with pytest.raises(ValueError, match="expected_travel_var"):
        cpm.Sampler.expected_travel_var(_NoDevice(), ok, ok, s_seconds=short, sparse=True)
    with pytest.raises(ValueError):
        cpm.Sampler.expected_linear_var(_NoDevice(), ok, ok, start=np.ones(5), sparse=True)
