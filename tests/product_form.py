"""Pins the kernel form that produced a step's results (not a conftest: imported by the tests that use it).

The blocking calls repair a failed step by themselves -- grown bucket regions, a one-launch hour that bailed out repeated with two
launches, a demotion to the exact layout -- and the repaired counts equal the oracle's.  A parity test that checks counts alone
has then tested some other kernel than the one it names.  `pinned` wraps one step (an IVP or a resample) and checks the
context's record of it (cpm_get_info: CPM_INFO_LAST_KERNEL, _LAST_FORM, _STEPS_REPEATED, _CAP_MULT, _PARTS, _FUSED_BAILOUTS):

    with pinned(s, kernel=5, fused=1):
        r = s.resample(seed)

  kernel    the kernel setting of the context (CPM_OPT_KERNEL): an explicit family must be the one that ran; AUTO must be what the
            library's rule picks (restated here: fewer than 32 of the context's cars per zone -> the per-car kernel, otherwise the
            grouped path, which fits every problem these tests pin).  `family` overrides the expectation (fallback tests).
  fused     the CPM_OPT_FUSED mode the test set (5, the library's default, when it set none).  A forced mode must run its form
            (MODE_FORM); under 5 the form is what CPM_INFO_FUSED predicted just before the step.  `form` names the literal value
            where a test means one: asserted always for a forced mode, on 256-CU devices only under 5 (where it pays depends on the
            CU count).
  repeats   discarded-and-repeated attempts in this step: an int (exact), at_least(n), or None (not checked).  Default 0.
  bailouts  steps that bailed out of a one-launch form during this step, likewise.  Default 0.
  cap_mult, parts   CPM_INFO_CAP_MULT / _PARTS after the step, where they matter (int, at_least(n) or None).

The deltas are read around the step, so several pinned steps can share one context.  The yielded dict is filled with the record
after the step (Sampler.last_step(), plus `step_repeats` / `step_bailouts`, the deltas).
"""
import contextlib
import functools

from carparkingmaps_amd import _lib

CAR, ZONE_LDS, GROUPED = _lib.CPM_KERNEL_CAR, _lib.CPM_KERNEL_ZONE_LDS, _lib.CPM_KERNEL_ZONE_GROUPED
# CPM_OPT_FUSED mode -> CPM_INFO_LAST_FORM of a step that ran it (2, 4, 7 are the bail-out modes: their form until they bail)
MODE_FORM = {0: 0, 1: 1, 2: 1, 3: 3, 4: 3, 6: 6, 7: 6, 8: 6}


class at_least:
    def __init__(self, n):
        self.n = n

    def ok(self, v):
        return v >= self.n

    def __repr__(self):
        return f">= {self.n}"


def _ok(want, got):
    return want is None or (want.ok(got) if isinstance(want, at_least) else got == want)


@functools.lru_cache(maxsize=None)
def cu_count(device=0):
    from carparkingmaps_amd import device_info
    return device_info(device)["cu_count"]


def auto_family(s):
    """The family AUTO picks for the context's cars (pick_kernel in csrc/cpm_api.hip, restated)."""
    return CAR if s.car_count < 32 * s.Z else GROUPED


def expected_family(s, kernel):
    return auto_family(s) if kernel == _lib.CPM_KERNEL_AUTO else kernel


@contextlib.contextmanager
def pinned(s, kernel=_lib.CPM_KERNEL_AUTO, *, family=None, fused=5, form=None, repeats=0, bailouts=0, cap_mult=None, parts=None):
    before = s.last_step()
    predicted = s.get_info(_lib.CPM_INFO_FUSED)
    rec = {}
    yield rec
    after = s.last_step()
    rec.update(after, step_repeats=after["repeats"] - before["repeats"], step_bailouts=after["bailouts"] - before["bailouts"])
    where = f"step record {rec} (kernel setting {kernel}, fused mode {fused}, predicted form {predicted})"
    want_family = family if family is not None else expected_family(s, kernel)
    assert after["kernel"] == want_family, f"family {after['kernel']} produced the results, expected {want_family}: {where}"
    if want_family == GROUPED:
        if fused == 5:
            assert after["form"] == predicted, f"hour form {after['form']}, CPM_INFO_FUSED predicted {predicted}: {where}"
            if form is not None and cu_count() == 256:
                assert after["form"] == form, f"hour form {after['form']}, expected {form} on 256 CUs: {where}"
        else:
            want_form = form if form is not None else MODE_FORM[fused]
            assert after["form"] == want_form, f"hour form {after['form']}, fused mode {fused} expects {want_form}: {where}"
    else:
        assert after["form"] == -1, f"hour form {after['form']} reported for family {after['kernel']}: {where}"
    assert _ok(repeats, rec["step_repeats"]), f"{rec['step_repeats']} repeated attempts, expected {repeats!r}: {where}"
    assert _ok(bailouts, rec["step_bailouts"]), f"{rec['step_bailouts']} bail-outs, expected {bailouts!r}: {where}"
    assert _ok(cap_mult, after["cap_mult"]), f"CAP_MULT {after['cap_mult']}, expected {cap_mult!r}: {where}"
    assert _ok(parts, after["parts"]), f"PARTS {after['parts']}, expected {parts!r}: {where}"
