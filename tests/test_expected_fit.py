"""Value and four-parameter gradient of the noise-free objectives (include/cpm_expected_fit.h), without a GPU: the ABI list, the
header under a strict C compiler, the entries without a device, the numpy restatement of the header (tests/expected_fit_reference.py)
against the host's own cotangent and chain-rule functions and against central differences, and what Evaluator.expected_fit and
refine_expected refuse before they touch the sampler."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import expected_fit_reference as ref

ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_set_measured_activity", "cpm_expected_fit_dev", "cpm_expected_fit"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_fit.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_FIT_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "EXPECTED_FIT_SYMBOLS"]
    assert len(others) >= 13
    for other in others:
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_fit.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_expected_fit.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_FIT_H", "CPM_FIT_DEST", "CPM_FIT_WORDS"]   # no new option, info key or status
    assert '#include "cpm_expected_grad_batch.h"' in text
    # CPM_FIT_DEST collides with no CPM_EXPECT_* bit
    bits = 0
    for header in os.listdir(os.path.join(ROOT, "include")):
        for name, value in re.findall(r"#define (CPM_EXPECT_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?", open(os.path.join(ROOT, "include", header)).read()):
            bits |= int(value, 0)
    assert bits & 1 and _lib.CPM_FIT_DEST & bits == 0 and _lib.CPM_FIT_DEST & (_lib.CPM_FIT_DEST - 1) == 0
    assert int(re.search(r"#define CPM_FIT_DEST (0x[0-9a-f]+)u", text).group(1), 16) == _lib.CPM_FIT_DEST
    assert int(re.search(r"#define CPM_FIT_WORDS (\d+)", text).group(1)) == _lib.CPM_FIT_WORDS == ref.FIT_WORDS == 16
    for method in ("set_measured_activity", "expected_fit_dev", "expected_fit", "fit_words"):
        assert getattr(cpm.Sampler, method)


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_fit_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_fit.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[CPM_FIT_WORDS + 4] = {0};
    int32_t r[3];
    int i;
    r[0] = cpm_set_measured_activity(ctx, a);
    r[1] = cpm_expected_fit_dev(ctx, 1, a, a, a, NULL, CPM_EXPECT_IVP | CPM_FIT_DEST, a, a, NULL, NULL, NULL, NULL);
    r[2] = cpm_expected_fit(ctx, 1, a, a, a, NULL, 0u, a, a, NULL, NULL, NULL, NULL);
    for (i = 1; i < 3; ++i) if (r[i] != r[0]) return 1;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_fit_header")
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
    assert L.cpm_set_measured_activity(None, vp) == want
    assert L.cpm_set_measured_activity(None, None) == want
    for flags in (0, _lib.CPM_EXPECT_IVP, _lib.CPM_FIT_DEST, _lib.CPM_EXPECT_IVP | _lib.CPM_FIT_DEST):
        assert L.cpm_expected_fit_dev(None, 1, vp, vp, vp, None, flags, vp, vp, None, None, None, None) == want
        assert L.cpm_expected_fit(None, 1, vp, vp, vp, None, flags, vp, vp, None, None, None, None) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()


# ------------------------------------------------------------------ the reference against the host functions
def _case(seed, Z, T):
    """random (T, Z) densities with a flat zone, an unmeasured zone and a tie of the minimum planted"""
    rng = np.random.default_rng(seed)
    p = rng.random((T, Z)) / Z
    x = p * rng.random((T, Z))
    m_p = rng.random((T, Z))
    if Z >= 3:
        p[:, 1] = p[0, 1]            # flat
        m_p[:, 2] = 0.0              # unmeasured
    p[T - 1, 0] = p[:, 0].min()      # the minimum twice: the first hour counts
    m_a = rng.random(T)
    w_sec = 300.0 + 900.0 * rng.random((T, Z))
    return p, x, m_a, m_p, w_sec


SHAPES = [(2, 24), (5, 24), (67, 5), (300, 24), (1031, 7)]


@pytest.mark.parametrize("Z,T", SHAPES)
def test_reference_cotangents_match_the_host_functions(cpm, Z, T):
    from carparkingmaps_amd import model_selection as ms
    p, x, m_a, m_p, w_sec = _case(1000 + Z, Z, T)
    total = float((x * w_sec).sum())
    w = (0.7, 1.3, 2.1)
    r = ref.fit_reference(p, x, w, m_a, m_p, w_sec, total)
    valid_host = (m_p.sum(axis=0) != 0) & (p.max(axis=0) != p.min(axis=0))
    assert (r["valid"] == valid_host).all() and r["n_valid"] >= 1
    assert Z < 3 or r["n_valid"] <= Z - 2          # the flat and the unmeasured zone
    g_act = ms.traffic_activity_error_grad(x.T, m_a).T
    g_park = ms.parking_density_error_grad(p.T, m_p.T).T
    g_adr = ms.a_drive_grad(w_sec.T).T
    tol = 8 * (T + Z) * 2.0 ** -53
    # each term against its host function, relative to the magnitude sums of the terms it is made of
    one = ref.fit_reference(p, x, (1.0, 0.0, 0.0), m_a, m_p, w_sec, total)
    mag_act = np.abs(g_act).max() * T                        # (every word holds a sum over the T hours: s1, s2)
    assert np.abs(one["g_driving"] - g_act).max() <= tol * mag_act and not one["g_parking"].any()
    one = ref.fit_reference(p, x, (0.0, 1.0, 0.0), m_a, m_p, w_sec, total)
    mag_park = np.abs(g_park).max(axis=0) * T
    assert (np.abs(one["g_parking"] - g_park).max(axis=0) <= tol * mag_park).all() and not one["g_driving"].any()
    assert not one["g_parking"][:, ~valid_host].any()
    one = ref.fit_reference(p, x, (0.0, 0.0, 1.0), m_a, m_p, w_sec, total)
    assert np.abs(one["g_driving"] - g_adr).max() <= tol * np.abs(g_adr).max() and not one["g_parking"].any()
    # the weighted sum
    mix_d, mix_p = w[0] * g_act + w[2] * g_adr, w[1] * g_park
    assert np.abs(r["g_driving"] - mix_d).max() <= tol * (w[0] * mag_act + w[2] * np.abs(g_adr).max())
    assert (np.abs(r["g_parking"] - mix_p).max(axis=0) <= tol * w[1] * mag_park).all()
    # the values against expected_objectives
    o = ms.expected_objectives(p.T, x.T, m_a, m_p.T, seconds=total)
    assert abs(r["activity_error"] - o["activity_error"]) <= tol * 4 * max(1.0, o["activity_error"]) * (x.sum(axis=1).max() / np.ptp(x.sum(axis=1)))
    assert abs(r["parking_error"] - o["parking_error"]) <= tol * o["parking_error"]
    assert r["A_drive"] == o["A_drive"]
    assert abs(r["F"] - (w[0] * o["activity_error"] + w[1] * o["parking_error"] + w[2] * o["A_drive"])) <= tol * 8 * abs(r["F"]) * (
        x.sum(axis=1).max() / np.ptp(x.sum(axis=1)))


def test_reference_zero_weight_does_not_form_a_nan_term_and_flat_cases_give_zero(cpm):
    p, x, m_a, m_p, w_sec = _case(7, 5, 24)
    r = ref.fit_reference(p, x, (1.0, 0.0, 0.5), m_a, None, w_sec, 10.0)     # no measured parking: parking_error NaN, not weighed
    assert np.isnan(r["parking_error"]) and r["n_valid"] == 0 and np.isfinite(r["F"]) and not r["g_parking"].any()
    flat = np.full_like(x, 0.25)
    r = ref.fit_reference(p, flat, (0.0, 1.0, 0.0), m_a, m_p, w_sec, 10.0)   # a flat activity: NaN, zero cotangent
    assert np.isnan(r["activity_error"]) and np.isnan(r["traffic_activity"]).all() and not r["ga"].any() and np.isfinite(r["F"])


@pytest.mark.parametrize("Z,T", [(5, 24), (67, 5)])
def test_reference_cotangents_match_central_differences(cpm, Z, T):
    """Judged by the differences' own truncation error, as tests/test_expected_grad.py does: the derivative from two step sizes, the
    gap between them bounding the error of the finer one.  Entries at an argmin / argmax (a kink of the min-max normalisation) are
    skipped for the term they are a kink of."""
    from carparkingmaps_amd import model_selection as ms
    p, x, m_a, m_p, w_sec = _case(2000 + Z, Z, T)
    p[T - 1, 0] = p[:, 0].max() * 1.5     # (no tie here: a tie is a kink)
    total = float((x * w_sec).sum())
    w = (0.7, 1.3, 2.1)
    r = ref.fit_reference(p, x, w, m_a, m_p, w_sec, total)

    def F(pp, xx):
        o = ms.expected_objectives(pp.T, xx.T, m_a, m_p.T, seconds=float((xx * w_sec).sum()))
        return w[0] * o["activity_error"] + w[1] * o["parking_error"] + w[2] * o["A_drive"]

    rng = np.random.default_rng(5)
    a = x.sum(axis=1)
    checked = 0
    for which, arr, g in (("p", p, r["g_parking"]), ("x", x, r["g_driving"])):
        for _ in range(12):
            t, z = int(rng.integers(T)), int(rng.integers(Z))
            if which == "p" and (t in (p[:, z].argmin(), p[:, z].argmax()) or not r["valid"][z]):
                continue
            if which == "x" and t in (a.argmin(), a.argmax()):
                continue
            ds = []
            for h in (1e-5 * arr[t, z], 5e-6 * arr[t, z]):
                up, dn = arr.copy(), arr.copy()
                up[t, z] += h
                dn[t, z] -= h
                ds.append((F(up, x) - F(dn, x)) / (2 * h) if which == "p" else (F(p, up) - F(p, dn)) / (2 * h))
            err = abs(ds[0] - ds[1]) + 1e-9 * abs(ds[1]) + 2.0 ** -53 * abs(F(p, x)) / (5e-6 * arr[t, z]) * 4
            assert abs(g[t, z] - ds[1]) <= err, (which, t, z, g[t, z], ds)
            checked += 1
    assert checked >= 8


def test_reference_chain_rule_matches_the_host_functions(cpm):
    from carparkingmaps_amd import model_selection as ms
    rng = np.random.default_rng(11)
    T, Z = 24, 67
    s = rng.random((T, Z))
    s[3, 5] = 0.0
    g = rng.standard_normal((T, Z))
    g[rng.random((T, Z)) < 0.2] = 0.0
    gd = rng.standard_normal((T, Z))
    x, dw = rng.random((T, Z)) / Z, rng.standard_normal((T, Z))
    on = np.ones(Z, dtype=bool)
    for e in (0.5, 1.0, 2.0, 0.73):
        vals, mags = ref.chain_rule_mp(g, s, on, 0.1, 0.8, e, gd, x, dw, w_adrive=1.0)
        host = ms.p_drive_param_grads(g.T, s.T, 0.1, 0.8, e) + (ms.e_dest_param_grad(gd.T, x.T, dw.T),)
        for v, m, h in zip(vals, mags, host):
            assert abs(float(v) - h) <= 4 * T * Z * 2.0 ** -53 * float(m), (e, float(v), h)
    vals, _ = ref.chain_rule_mp(g, s, on, 0.1, 0.8, 0.73)
    assert vals[3] is None
    # the two-stage sum is a sum
    v = rng.random(T * Z)
    assert abs(ref.chunk_sum(v) - v.sum()) <= 32 * 2.0 ** -53 * v.sum()
    assert abs(float(ref.zone_sum(v)) - v.sum()) <= ref.zone_sum_bound(v.size) * v.sum() + 8 * 2.0 ** -53 * v.sum()


# ------------------------------------------------------------------ refusals before the sampler is touched
class _Untouchable:
    """a sampler that fails the test on any use"""
    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched: {name}")


def test_evaluator_and_refine_refuse_before_they_touch_the_sampler(cpm):
    from carparkingmaps_amd import model_selection as ms
    ev = ms.Evaluator(_Untouchable(), C=1, seed=1, measured_activity=np.zeros(24), measured_parking=None)
    same = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(0.6, 0.2, 0.8, 2)]
    mixed = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(0.5, 0.1, 0.9, 1.5)]
    for call in (ev.expected_fit, lambda pts, weights=None, **kw: ms.refine_expected(ev, pts, weights, **kw)):
        with pytest.raises(ValueError, match="share e_dest"):
            call(mixed, {"activity_error": 1.0})
        with pytest.raises(ValueError, match="unknown weight keys"):
            call(same, {"a_drive": 1.0})
        with pytest.raises(ValueError, match="measured_parking"):
            call(same, {"parking_error": 1.0})
        with pytest.raises(ValueError, match="measured_parking"):
            call(same, [{"activity_error": 1.0}, {"parking_error": 0.5}])
        with pytest.raises(ValueError, match="weight dicts"):
            call(same, [{"activity_error": 1.0}])
    ev2 = ms.Evaluator(_Untouchable(), C=1, seed=1, measured_activity=None, measured_parking=np.ones((3, 24)))
    with pytest.raises(ValueError, match="measured_activity"):
        ev2.expected_fit(same)
    with pytest.raises(ValueError, match="bounds that cross"):
        ms.refine_expected(ev, same, {"activity_error": 1.0}, bounds={"p_min": (0.5, 0.2)})
    with pytest.raises(ValueError, match="bounds that cross"):
        ms.refine_expected(ev, same, {"activity_error": 1.0}, bounds={"p_min": (0.9, 1.0), "p_max": (0.0, 0.5)})
    with pytest.raises(ValueError, match="unknown bound"):
        ms.refine_expected(ev, same, {"activity_error": 1.0}, bounds={"e_dest": (1.0, 2.0)})
