"""The batched adjoint of the expected densities (include/cpm_expected_grad_batch.h), without a GPU: the ABI list, the header under a
strict C compiler, the entries without a device, and what Evaluator.expected_gradient_batch refuses before it touches the sampler."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG, ERR_HIP = -1, -2
NEW = ["cpm_expected_grad_batch_dev", "cpm_expected_grad_batch", "cpm_expected_grad_dest_batch_dev", "cpm_expected_grad_dest_batch"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def _no_device(L):
    n = ctypes.c_int32(0)
    return L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared("cpm_expected_grad_batch.h")
    assert declared == sorted(NEW) == sorted(_lib.EXPECTED_GRAD_BATCH_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.FLOWS_SYMBOLS, _lib.FLOWS_CSR_SYMBOLS, _lib.STAYS_SYMBOLS, _lib.PATHS_SYMBOLS,
                  _lib.CHARGE_SYMBOLS, _lib.OBJECTIVES_SYMBOLS, _lib.EXPECTED_SYMBOLS, _lib.EXPECTED_TRAVEL_SYMBOLS, _lib.EXPECTED_GRAD_SYMBOLS,
                  _lib.EXPECTED_GRAD_DEST_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_expected_grad_batch.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_expected_grad_batch.h")).read()
    assert re.findall(r"#define (CPM_\w+)", text) == ["CPM_EXPECTED_GRAD_BATCH_H"]   # no new option, info key or flag
    assert '#include "cpm_expected_grad_dest.h"' in text
    for method in ("expected_grad_batch", "expected_grad_batch_dev", "expected_grad_dest_batch_dev"):
        assert getattr(cpm.Sampler, method)
    # the two B = 1 headers point here instead of stating the restriction
    for header in ("cpm_expected_grad.h", "cpm_expected_grad_dest.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "B = 1 only" not in text and "cpm_expected_grad_batch.h" in text, header


def test_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "expected_grad_batch_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_expected_grad_batch.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    double a[4] = {0};
    int32_t r[4];
    int i;
    r[0] = cpm_expected_grad_batch_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL, a, NULL);
    r[1] = cpm_expected_grad_batch(ctx, NULL, 0u, a, a, NULL, a, NULL);
    r[2] = cpm_expected_grad_dest_batch_dev(ctx, NULL, CPM_EXPECT_IVP, a, NULL, a, NULL, a);
    r[3] = cpm_expected_grad_dest_batch(ctx, NULL, 0u, a, a, NULL, a, NULL, a);
    for (i = 1; i < 4; ++i) if (r[i] != r[0]) return 1;
    return r[0] == CPM_ERR_HIP ? 0 : r[0] == CPM_ERR_ARG ? 2 : 3;   /* no device | a device and a null context */
}
""")
    exe = str(tmp_path / "expected_grad_batch_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    # whether a fresh process sees a device: the program is one, and this process may hold another HIP runtime by now
    probe = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); n = ctypes.c_int32(0); "
             "sys.exit(0 if L.cpm_device_count(ctypes.byref(n)) != 0 or n.value < 1 else 2)")
    want = subprocess.run([sys.executable, "-c", probe, _lib.LIB_PATH]).returncode
    assert want in (0, 2) and subprocess.run([exe]).returncode == want


def test_every_entry_returns_err_hip_without_a_device(cpm):
    from carparkingmaps_amd import _lib
    L = _lib.load()
    a = np.zeros(8)
    vp = a.ctypes.data_as(ctypes.c_void_p)
    want = ERR_HIP if _no_device(L) else ERR_ARG
    for flags in (0, _lib.CPM_EXPECT_IVP):
        assert L.cpm_expected_grad_batch_dev(None, None, flags, vp, None, vp, None) == want
        assert L.cpm_expected_grad_batch(None, None, flags, vp, vp, None, vp, None) == want
        assert L.cpm_expected_grad_dest_batch_dev(None, None, flags, vp, None, vp, None, vp) == want
        assert L.cpm_expected_grad_dest_batch(None, None, flags, vp, vp, None, vp, None, vp) == want
    assert (b"no HIP device" if want == ERR_HIP else b"null context") in L.cpm_last_error()


class _Untouchable:
    """a sampler that fails the test on any use"""
    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched: {name}")


def test_evaluator_refuses_before_it_touches_the_sampler(cpm):
    from carparkingmaps_amd import model_selection as ms
    ev = ms.Evaluator(_Untouchable(), C=1, seed=1, measured_activity=np.zeros(24), measured_parking=None)
    same = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(0.6, 0.2, 0.8, 2)]
    mixed = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(0.5, 0.1, 0.9, 1.5)]
    with pytest.raises(ValueError, match="unknown objective"):
        ev.expected_gradient_batch(same, "a_drive")
    for objective in ("activity_error", "parking_error", "A_drive"):
        for dest in (False, True):
            with pytest.raises(ValueError, match="share e_dest"):
                ev.expected_gradient_batch(mixed, objective, dest=dest)
    with pytest.raises(ValueError, match="measured_parking"):
        ev.expected_gradient_batch(same, "parking_error")
