"""The backward operator and the trip weights from the compact rows (include/cpm_expected_sparse_grad.h), without a GPU: the order of
the dense kernels' sums restated in numpy with every destination, zeros included, against the order of the sparse kernels over the
stored cells alone -- equal in every bit and in the sign of every zero -- at the sizes that cover the segments' geometry; two mutant
orders that must differ; the header, the exports and the refusals that need no device."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1031, 1089]
TC = 2
ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_expected_sparse_grad_dev", "cpm_expected_sparse_grad", "cpm_expected_sparse_grad_batch_dev", "cpm_expected_sparse_grad_batch",
       "cpm_expected_sparse_trip_dev", "cpm_expected_sparse_trip", "cpm_expected_sparse_travel_dev", "cpm_expected_sparse_travel",
       "cpm_expected_sparse_travel_batch", "cpm_expected_sparse_fit_dev", "cpm_expected_sparse_fit"]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(np.signbit(a), np.signbit(b))


@functools.lru_cache(maxsize=None)
def _case(Z):
    """the hand-made tables, the kept cells of weight 0, the cotangent, the means and the distances of one size: computed once, shared"""
    _, p_dest, info = S.sparse_tables(Z, TC)
    rng = np.random.default_rng(1000 + Z)
    mean = rng.uniform(-50.0, 3000.0, (Z, Z, TC))          # (negative means are fine)
    mean[Z - 1, 0, :] = -7.5                               # ... and one is there at every size
    dist = rng.uniform(0.1, 40.0, (Z, Z))
    hours = []
    for t in range(TC):
        p_t = np.ascontiguousarray(p_dest[:, :, t])
        keep = G.kept_zero_cells(p_t)
        hours.append((p_t, G.rows_of(p_t, keep), keep))
    return hours, G.cotangent(Z, TC), mean, dist, info


# ------------------------------------------------------------------ the geometry
def test_segment_counts_are_pinned_and_cover_the_geometry():
    want = {2: (1, 2), 3: (1, 3), 4: (1, 4), 5: (1, 5), 31: (1, 31), 32: (1, 32), 33: (1, 33), 63: (1, 63), 64: (2, 32), 65: (2, 33),
            127: (3, 43), 128: (4, 32), 129: (4, 33), 1031: (32, 33), 1089: (34, 33)}
    got = {Z: (G.grad_segments(Z), G.segment_len(Z, G.grad_segments(Z))) for Z in SIZES}
    assert got == want
    assert min(n for n, _ in got.values()) == 1 and max(n for n, _ in got.values()) == 34
    assert {l % 4 for _, l in got.values()} == {0, 1, 2, 3}
    assert 1031 - 31 * 33 == 8                                                          # the last segment of 1,031 has 8 destinations
    empty = [Z for Z in range(2, 1090) if (G.grad_segments(Z) - 1) * G.segment_len(Z, G.grad_segments(Z)) >= Z]
    assert empty == [1089] and 1089 in SIZES                                            # an empty trailing segment first happens there
    assert [G.trip_segments(Z, TC) for Z in SIZES] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 8, 8]
    assert G.trip_segments(358, 24) == 6 and G.trip_segments(2357, 24) == 3 and G.trip_segments(1089, 3) == 8
    assert G.grad_segments(2357) == 54 and G.segment_len(2357, 54) == 44                # Melbourne: seg_len % 4 == 0
    assert G.grad_segments(4096) == 32 and G.grad_segments(358) == 11


def test_the_cases_hold_what_they_are_meant_to():
    hours, mu, _, _, info = _case(129)
    p_t, rows, keep = hours[0]
    assert (mu < 0).any() and (mu == 0).any() and not mu[TC - 1].any() and mu[0].any()
    assert not p_t[info["zero"]].any() and all(len(rows[o]) == 0 or all(p == 0 for _, p in rows[o]) for o in info["zero"])
    assert (hours[TC - 1][0][:, info["full"]] > 0).all() and not p_t[:, info["empty"]].any()
    before = behind = 0
    for o, d in keep:
        last = max(dd for dd, p in rows[o] if p > 0)
        before += d < last
        behind += d > last
        assert (d, 0.0) in rows[o]
    assert before > 0 and behind > 0
    assert all(r == sorted(r) and len({d for d, _ in r}) == len(r) for r in rows)


# ------------------------------------------------------------------ the two orders
@pytest.mark.parametrize("Z", SIZES)
def test_sparse_order_gives_the_bits_of_the_dense_order(Z):
    hours, mu, mean, dist, _ = _case(Z)
    nseg = G.grad_segments(Z)
    for t, (p_t, rows, _) in enumerate(hours):
        dense = G.dense_u(p_t, mu[t])
        sparse = G.sparse_u(rows, mu[t], Z)
        assert dense.shape == (nseg, Z) and _bits_equal(dense, sparse), (Z, t)
        assert not np.signbit(dense[dense == 0.0]).any()                                # a chain never becomes -0
        assert _bits_equal(G.finish(dense), G.finish(sparse))
    assert not G.dense_u(hours[TC - 1][0], mu[TC - 1]).any()                            # the hour of all zeros


@pytest.mark.parametrize("Z", SIZES)
def test_sparse_trip_order_gives_the_bits_of_the_dense_order(Z):
    hours, _, mean, dist, _ = _case(Z)
    assert np.isfinite(mean).all() and np.isfinite(dist).all() and (mean < 0).any()     # the precondition of the header
    for t, (p_t, rows, _) in enumerate(hours):
        m_t = np.ascontiguousarray(mean[:, :, t])
        dense = G.dense_trip(p_t, m_t, dist, TC)
        sparse = G.sparse_trip(rows, m_t, dist, Z, TC)
        for a, b in zip(dense, sparse):
            assert _bits_equal(a, b), (Z, t)


def test_mutant_orders_differ_but_stay_close():
    Z = 1031                                                                            # seg_len = 33: begin & 3 != 0 for most segments
    hours, mu, _, _, _ = _case(Z)
    p_t, rows, _ = hours[0]
    good = G.sparse_u(rows, mu[0], Z)
    by_d = G.sparse_u(rows, mu[0], Z, chain=lambda d, begin: d & 3)
    assert not _bits_equal(good, by_d)
    u = G.finish(good)
    scale = np.abs(u).max()
    assert np.abs(G.finish(by_d) - u).max() <= 1e-12 * scale
    run = G.running_sum(rows, lambda o, d: mu[0][d], Z)
    assert not _bits_equal(u, run) and np.abs(run - u).max() <= 1e-12 * scale
    # at Melbourne's seg_len = 44 every segment begins at a multiple of 4: the first mutant would not show
    assert all((s * 44) & 3 == 0 for s in range(54))
    hours, mu, _, _, _ = _case(128)                                                     # seg_len = 32 likewise
    assert _bits_equal(G.sparse_u(hours[0][1], mu[0], 128), G.sparse_u(hours[0][1], mu[0], 128, chain=lambda d, begin: d & 3))


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
    declared = _declared("cpm_expected_sparse_grad.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_SPARSE_GRAD_SYMBOLS)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SYMBOLS") and k != "EXPECTED_SPARSE_GRAD_SYMBOLS"]
    assert len(others) >= 16
    for other in others:
        assert not set(declared) & set(other)
    L = _lib.load()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_sparse_grad.h but not exported"
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int32
    text = open(os.path.join(ROOT, "include", "cpm_expected_sparse_grad.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_SPARSE_GRAD_H"]     # no option, info key, status or flag of its own
    for h in os.listdir(os.path.join(ROOT, "include")):                                 # included from nowhere else
        if h != "cpm_expected_sparse_grad.h":
            assert "cpm_expected_sparse_grad.h" not in open(os.path.join(ROOT, "include", h)).read()
    for word in ("grad_segments", "(d - s * seg_len) & 3", "((w0 + w1) + w2) + w3", "1,089", "finite", "CPM_FIT_DEST"):
        assert word in text, word                                                       # the derivation and the preconditions are stated
    for method in ("expected_grad", "expected_grad_dev", "expected_grad_batch", "expected_grad_batch_dev", "expected_trip", "expected_trip_dev",
                   "expected_travel", "expected_travel_batch", "expected_travel_dev", "expected_fit", "expected_fit_dev"):
        assert inspect.signature(getattr(cpm.Sampler, method)).parameters["sparse"].default is False, method


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_sparse_grad_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_sparse_grad.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[8] = {0};
    int32_t r[11];
    int i;
    r[0] = cpm_expected_sparse_grad_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL, a, NULL);
    r[1] = cpm_expected_sparse_grad(ctx, NULL, 0u, a, a, NULL, a, NULL);
    r[2] = cpm_expected_sparse_grad_batch_dev(ctx, NULL, 0u, a, NULL, a, NULL);
    r[3] = cpm_expected_sparse_grad_batch(ctx, NULL, CPM_EXPECT_IVP, a, a, NULL, a, NULL);
    r[4] = cpm_expected_sparse_trip_dev(ctx, a);
    r[5] = cpm_expected_sparse_trip(ctx, a, a);
    r[6] = cpm_expected_sparse_travel_dev(ctx, a, 1, a, NULL);
    r[7] = cpm_expected_sparse_travel(ctx, NULL, 0u, a, a, NULL);
    r[8] = cpm_expected_sparse_travel_batch(ctx, NULL, 0u, a, a, a);
    r[9] = cpm_expected_sparse_fit_dev(ctx, 1, a, a, a, NULL, CPM_EXPECT_IVP, a, a, NULL, NULL, NULL, NULL);
    r[10] = cpm_expected_sparse_fit(ctx, 1, a, a, a, NULL, 0u, a, a, NULL, NULL, NULL, NULL);
    for (i = 1; i < 11; ++i) if (r[i] != r[0]) return 1;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_sparse_grad_header")
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
        assert L.cpm_expected_sparse_grad_dev(None, None, flags, vp, None, vp, None) == want
        assert L.cpm_expected_sparse_grad(None, None, flags, vp, vp, None, vp, None) == want
        assert L.cpm_expected_sparse_grad_batch_dev(None, None, flags, vp, None, vp, None) == want
        assert L.cpm_expected_sparse_grad_batch(None, None, flags, vp, vp, None, vp, None) == want
        assert L.cpm_expected_sparse_travel(None, None, flags, vp, vp, None) == want
        assert L.cpm_expected_sparse_travel_batch(None, None, flags, vp, vp, vp) == want
        assert L.cpm_expected_sparse_fit_dev(None, 1, vp, vp, vp, None, flags, vp, vp, None, None, None, None) == want
        assert L.cpm_expected_sparse_fit(None, 1, vp, vp, vp, None, flags, vp, vp, None, None, None, None) == want
    assert L.cpm_expected_sparse_trip_dev(None, vp) == want
    assert L.cpm_expected_sparse_trip(None, vp, vp) == want
    assert L.cpm_expected_sparse_travel_dev(None, vp, 1, vp, None) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()


class _NoDevice:
    """a Sampler whose library must not be reached: dest=True with sparse=True is refused before any device call"""
    Z, T = 4, 2

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came too late: {name} was touched")


def test_dest_with_sparse_is_refused_before_any_device_call(cpm):
    z = np.zeros((4, 2, 1))
    with pytest.raises(ValueError, match="dense array"):
        cpm.Sampler.expected_grad_batch(_NoDevice(), z, z, dest=True, sparse=True)
    with pytest.raises(ValueError, match="dense array"):
        cpm.Sampler.expected_fit(_NoDevice(), 0.1, 0.9, 0.5, [1.0, 0.0, 0.0], dest=True, sparse=True)
    with pytest.raises(ValueError, match="dense array"):
        cpm.Sampler.expected_fit_dev(_NoDevice(), 0.1, 0.9, 0.5, [1.0, 0.0, 0.0], 8, dest=True, sparse=True)
    from carparkingmaps_amd.model_selection import Evaluator
    assert "dest=True" in inspect.getsource(Evaluator).split("expected_sparse: bool")[0][-700:]   # the routing is stated where the switch is
