"""The e_dest direction from a compact tangent of p_destin (include/cpm_expected_sparse_dest.h), without a GPU: the order of the dense
kernel's sum of w restated in numpy with every destination, zeros included, against the order of the sparse kernel over the stored
cells alone -- equal in every bit and in the sign of every zero -- for SIGNED tangents; two mutant orders that must differ; the builder
against mpmath; the header, the exports and the refusals that need no device."""
import ctypes
import functools
import inspect
import os
import re
import subprocess
import sys

import mpmath
import numpy as np
import pytest

import expected_grad_dest_reference as D
import expected_sparse_dest_reference as SD
import expected_sparse_grad_reference as G
import expected_sparse_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 403, 518, 1031, 1089]
TC = 2
ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_build_p_dest_tangent_sparse", "cpm_set_p_dest_tangent_sparse", "cpm_get_p_dest_tangent_sparse", "cpm_expected_sparse_grad_dest_dev",
       "cpm_expected_sparse_grad_dest", "cpm_expected_sparse_grad_dest_batch_dev", "cpm_expected_sparse_grad_dest_batch",
       "cpm_expected_sparse_trip_tangent_dev", "cpm_expected_sparse_trip_tangent"]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(np.signbit(a), np.signbit(b))


@functools.lru_cache(maxsize=None)
def _case(Z):
    """the hand-made tables, the kept cells of weight 0, a signed tangent on the stored cells, the cotangent, the means and the distances
    of one size: computed once, shared"""
    _, p_dest, info = S.sparse_tables(Z, TC)
    rng = np.random.default_rng(2000 + Z)
    mean = rng.uniform(-50.0, 3000.0, (Z, Z, TC))
    mean[Z - 1, 0, :] = -7.5                                            # a negative mean at every size
    dist = rng.uniform(0.1, 40.0, (Z, Z))
    hours = []
    for t in range(TC):
        p_t = np.ascontiguousarray(p_dest[:, :, t])
        keep = G.kept_zero_cells(p_t)
        rows = G.rows_of(p_t, keep)
        dP_t, stored = SD.signed_tangent_on_cells(p_t, keep, 3000 + 7 * Z + t)
        hours.append((p_t, rows, keep, dP_t, SD.tangent_rows(rows, dP_t), stored))
    return hours, G.cotangent(Z, TC), mean, dist, info


def test_the_cases_hold_what_they_are_meant_to():
    for Z in (403, 1089):
        hours, mu, mean, _, info = _case(Z)
        p_t, rows, keep, dP_t, trows, stored = hours[0]
        assert (mu < 0).any() and (mu == 0).any() and not mu[TC - 1].any() and mu[0].any()     # negative, exact zeros, an hour of zero mu
        assert (dP_t < 0).any() and (dP_t > 0).any() and not dP_t[~stored].any()               # signed; +0 off the stored cells
        assert not np.signbit(dP_t[~stored]).any()
        assert np.abs(dP_t.sum(axis=1)).max() <= 1e-12                                         # rows sum to 0
        assert keep and all(p_t[o, d] == 0.0 and dP_t[o, d] != 0.0 for o, d in keep)           # kept cells of weight 0 carry a tangent
        assert all(not p_t[o].any() for o in info["zero"])                                     # zero rows
        assert all([d for d, _ in a] == [d for d, _ in b] for a, b in zip(rows, trows))        # entry for entry with the rows of p
        assert (mean < 0).any()
    assert G.grad_segments(1089) == 34 and 33 * G.segment_len(1089, 34) >= 1089                # an empty trailing segment


@pytest.mark.parametrize("Z", SIZES)
def test_sparse_order_of_w_gives_the_bits_of_the_dense_order(Z):
    hours, mu, _, _, _ = _case(Z)
    nseg = G.grad_segments(Z)
    for t, (p_t, rows, _, dP_t, trows, _) in enumerate(hours):
        dense = SD.dense_w(dP_t, mu[t])
        sparse = SD.sparse_w(trows, mu[t], Z)
        assert dense.shape == (nseg, Z) and _bits_equal(dense, sparse), (Z, t)
        assert not np.signbit(dense[dense == 0.0]).any()                                       # a chain of signed terms never becomes -0
        assert _bits_equal(G.finish(dense), G.finish(sparse))
        assert _bits_equal(G.dense_u(p_t, mu[t]), G.sparse_u(rows, mu[t], Z))                  # u beside it, from the same walk
    assert not SD.dense_w(hours[TC - 1][3], mu[TC - 1]).any()                                  # the hour of zero mu: +0 everywhere
    if Z > 2:
        assert SD.dense_w(hours[0][3], mu[0]).any()


@pytest.mark.parametrize("Z", SIZES)
def test_sparse_order_of_the_trip_tangent_gives_the_bits_of_the_dense_order(Z):
    hours, _, mean, dist, _ = _case(Z)
    assert np.isfinite(mean).all() and np.isfinite(dist).all() and (mean < 0).any()            # the precondition; a negative mean
    for t, (_, _, _, dP_t, trows, _) in enumerate(hours):
        m_t = np.ascontiguousarray(mean[:, :, t])
        for a, b in zip(SD.dense_trip_tan(dP_t, m_t, dist, TC), SD.sparse_trip_tan(trows, m_t, dist, Z, TC)):
            assert _bits_equal(a, b), (Z, t)


def test_mutant_orders_differ_but_stay_close():
    Z = 1031                                                                                   # seg_len = 33: begin & 3 != 0 for most segments
    hours, mu, _, _, _ = _case(Z)
    _, _, _, dP_t, trows, _ = hours[0]
    good = SD.sparse_w(trows, mu[0], Z)
    by_d = SD.sparse_w(trows, mu[0], Z, chain=lambda d, begin: d & 3)
    assert not _bits_equal(good, by_d)
    w = G.finish(good)
    scale = np.abs(dP_t).sum(axis=1).max() * np.abs(mu[0]).max()                               # the magnitude of the sum: the terms cancel
    assert np.abs(G.finish(by_d) - w).max() <= 1e-12 * scale
    run = G.running_sum(trows, lambda o, d: mu[0][d], Z)
    assert not _bits_equal(w, run) and np.abs(run - w).max() <= 1e-12 * scale


def test_builder_restated_in_numpy_meets_the_bound_against_mpmath():
    """k_exps_tan_cells' operations on rows of 1, 2, 40 and 309 cells with cells of weight 0 among them, against mpmath's value of the
    definition: within (n + 8) 2^-52 p (|l| + m~), the bound of include/cpm_expected_grad_dest.h"""
    mpmath.mp.prec = 200
    rng = np.random.default_rng(17)
    worst = 0.0
    for n, e in ((1, 2.0), (2, 0.5), (40, 1.7), (309, 2.0)):
        x = rng.uniform(1e-3, 1.0, n)
        x[0] = 1.0
        w = x ** e
        zero = rng.random(n) < 0.2
        zero[0] = False
        w[zero] = 0.0                                                                          # kept cells of weight 0
        p = w / w.sum()
        got = SD.build_row(x, p)
        exact, bound = D.tangent_mp(x, p)
        for d in range(n):
            if p[d] == 0.0:
                assert got[d] == 0.0 and not np.signbit(got[d])
                continue
            err = abs(mpmath.mpf(got[d]) - exact[d])
            assert bound[d] > 0 or err == 0
            if bound[d] > 0:
                worst = max(worst, float(err / bound[d]))
        if n > 1:
            assert abs(sum(got)) <= 1e-13                                                      # the rows of d / d e_dest sum to 0
    print(f"builder: worst error / bound {worst:.4f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ host side
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_sparse_dest.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_SPARSE_DEST_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "EXPECTED_SPARSE_DEST_SYMBOLS"]
    assert len(others) >= 17
    for other in others:
        assert not set(declared) & set(other)
    L = _lib.load()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_sparse_dest.h but not exported"
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int32
    text = open(os.path.join(ROOT, "include", "cpm_expected_sparse_dest.h")).read()
    assert re.findall(r"#define (CPM_\w+) ?(\d*)", text) == [("CPM_EXPECTED_SPARSE_DEST_H", ""), ("CPM_INFO_DEST_TANGENT_DENSE", "25"),
                                                             ("CPM_INFO_DEST_TANGENT_COMPACT", "26")]
    assert (_lib.CPM_INFO_DEST_TANGENT_DENSE, _lib.CPM_INFO_DEST_TANGENT_COMPACT) == (25, 26)
    taken = set()
    for h in os.listdir(os.path.join(ROOT, "include")):                                        # the two info words are numbers not in use
        if h != "cpm_expected_sparse_dest.h":
            taken |= {int(v) for v in re.findall(r"#define CPM_INFO_\w+ (\d+)", open(os.path.join(ROOT, "include", h)).read())}
    assert taken and not taken & {25, 26}
    for word in ("(d - s * seg_len) & 3", "((w0 + w1) + w2) + w3", "1,089", "finite", "CPM_FIT_DEST", "CPM_ERR_TABLE", "off the stored cells"):
        assert word in text, word
    for method in ("set_p_dest_tangent", "build_p_dest_tangent", "get_p_dest_tangent", "expected_grad_dest", "expected_grad_dest_dev",
                   "expected_grad_dest_batch_dev", "expected_trip_tangent", "expected_trip_tangent_dev"):
        assert inspect.signature(getattr(cpm.Sampler, method)).parameters["sparse"].default is False, method
    for method in ("expected_grad_batch", "expected_fit", "expected_fit_dev"):
        assert inspect.signature(getattr(cpm.Sampler, method)).parameters["compact_tangent"].default is False, method


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_sparse_dest_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_sparse_dest.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[8] = {0};
    int32_t r[9];
    int i;
    r[0] = cpm_build_p_dest_tangent_sparse(ctx);
    r[1] = cpm_set_p_dest_tangent_sparse(ctx, a);
    r[2] = cpm_get_p_dest_tangent_sparse(ctx, a);
    r[3] = cpm_expected_sparse_grad_dest_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL, a, NULL, a);
    r[4] = cpm_expected_sparse_grad_dest(ctx, NULL, 0u, a, a, NULL, a, NULL, a);
    r[5] = cpm_expected_sparse_grad_dest_batch_dev(ctx, NULL, 0u, a, NULL, a, NULL, a);
    r[6] = cpm_expected_sparse_grad_dest_batch(ctx, NULL, CPM_EXPECT_IVP, a, a, NULL, a, NULL, a);
    r[7] = cpm_expected_sparse_trip_tangent_dev(ctx, a);
    r[8] = cpm_expected_sparse_trip_tangent(ctx, a, a);
    for (i = 1; i < 9; ++i) if (r[i] != r[0]) return 1;
    if (CPM_INFO_DEST_TANGENT_DENSE == CPM_INFO_DEST_TANGENT_COMPACT || (CPM_FIT_DEST & CPM_EXPECT_IVP)) return 4;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_sparse_dest_header")
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
    z = np.zeros((4, 2, 1))
    fit = (0.1, 0.9, 0.5, [1.0, 0.0, 0.0])
    # compact_tangent=False keeps today's refusal of dest with sparse
    with pytest.raises(ValueError, match="dense array"):
        cpm.Sampler.expected_grad_batch(_NoDevice(), z, z, dest=True, sparse=True, compact_tangent=False)
    with pytest.raises(ValueError, match="dense array"):
        cpm.Sampler.expected_fit(_NoDevice(), *fit, dest=True, sparse=True)
    with pytest.raises(ValueError, match="dense array"):
        cpm.Sampler.expected_fit_dev(_NoDevice(), *fit, 8, dest=True, sparse=True)
    # compact_tangent=True without sparse=True
    with pytest.raises(ValueError, match="sparse=True"):
        cpm.Sampler.expected_grad_batch(_NoDevice(), z, z, dest=True, compact_tangent=True)
    with pytest.raises(ValueError, match="sparse=True"):
        cpm.Sampler.expected_fit(_NoDevice(), *fit, dest=True, compact_tangent=True)
    with pytest.raises(ValueError, match="sparse=True"):
        cpm.Sampler.expected_fit_dev(_NoDevice(), *fit, 8, dest=True, compact_tangent=True)
    # with both, the call goes on to the library
    with pytest.raises(AssertionError, match="was touched"):
        cpm.Sampler.expected_fit_dev(_NoDevice(), *fit, 8, dest=True, sparse=True, compact_tangent=True)
    from carparkingmaps_amd.model_selection import Evaluator
    with pytest.raises(ValueError, match="expected_sparse=True"):
        Evaluator(_NoDevice(), 1, 1, expected_sparse_dest=True)
    ev = Evaluator(_NoDevice(), 1, 1, expected_sparse=True, expected_sparse_dest=True)
    assert ev._sparse(True) and ev._sparse(False)
    assert not Evaluator(_NoDevice(), 1, 1, expected_sparse=True)._sparse(True)
    for name in ("expected_jacobian",):
        assert "dense tangent" in inspect.getdoc(getattr(Evaluator, name)).lower()
    from carparkingmaps_amd import model_selection as M
    assert "dense tangent" in inspect.getdoc(M.refine_expected_lm)
