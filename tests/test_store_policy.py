"""The bucket ids that only the next launch reads -- the stayers of the sampler workgroups, the arrivals of the placing blocks (sorted
write-out, medium runs, surplus) -- cross every hourly kernel boundary through stores whose cache policy is chosen per form of the
hour, as is the cache policy of the row pack's stream (csrc/cpm_grouped.h: next_store, store_policy, pack_dma;
profiles/store_policy_notes.md).  Whatever the policy, the next launch must find
every id: parity with the oracle on shapes that reach every one of those store sites, in the one-launch hour and in the two
launches per hour, each step pinned to its form; and two resamples enqueued back to back on the context's stream, with no host
synchronisation between them, must agree -- the second one's first launch reads what the first one's last launches stored.
Run on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

from conftest import SIM_SEED, TABLE_SEED
from product_form import pinned

pytestmark = pytest.mark.gpu

# (Z, cars per zone, T, sparse tables)
#   700 x 300    several chunks of 64 origin zones, the last one partial; every bucket inside a workgroup's slots
#   130 x 1,100  buckets beyond a workgroup's slots (the overflow round's stayer store) and runs beyond 64 entries (medium and surplus stores)
#   2,357 x 150  sparse row packs (a datamatrix of density 0.3, as test_fused_hour_equals_two_launches_per_hour builds them)
SHAPES = [(700, 300, 6, False), (130, 1100, 6, False), (2357, 150, 4, True)]


def _zone0(C, cpz):
    return np.arange(C, dtype=np.int64) // cpz + 1


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"{p[0]}x{p[1]}" + ("-sparse" if p[3] else ""))
def case(request, cpm, O):
    """One context per shape with its tables installed, and the oracle's run of it (computed once, shared, never written to)."""
    import torch
    Z, cpz, T, sparse = request.param
    C = Z * cpz
    s = cpm.Sampler(Z, T, stream=torch.cuda.Stream())
    try:
        if sparse:
            dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.3)
            s.set_datamatrix(dm, dist)
            p_drive = s.build_p_drive(0.1, 0.9, 0.5)
            p_dest = s.build_p_dest(2)
        else:
            p_drive, p_dest = O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED)
            s.set_p_drive(p_drive)
            s.set_p_dest(p_dest)
        ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz))
        for a in (ref["parking"], ref["driving"], ref["zone0"]):
            a.setflags(write=False)
        s.set_kernel(5)
        yield dict(s=s, Z=Z, cpz=cpz, T=T, C=C, ref=ref)
    finally:
        s.close()


@pytest.mark.parametrize("mode", [1, 0], ids=["one-launch", "two-launches"])
def test_ids_cross_the_hourly_boundary(cpm, case, mode):
    import torch
    from carparkingmaps_amd.distributed import split_counts
    s, Z, T, C, cpz, ref = case["s"], case["Z"], case["T"], case["C"], case["cpz"], case["ref"]
    s.set_fused(mode)
    s.init_states(C, cpz)
    # pinned: the form the mode names produced the results -- no step repeated, no bail-out, bucket regions of 4 x the mean bucket
    with pinned(s, 5, fused=mode, cap_mult=4):
        assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
    with pinned(s, 5, fused=mode, cap_mult=4):
        r = s.resample(SIM_SEED)
    assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"])
    # two resamples back to back on the context's stream, no host synchronisation in between
    with pinned(s, 5, fused=mode, cap_mult=4):
        with torch.cuda.stream(s._stream_obj):
            a = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda")
            b = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda")
            s.resample_dev(SIM_SEED, a.data_ptr())
            s.resample_dev(SIM_SEED, b.data_ptr())
            ha, hb = a.cpu(), b.cpu()
    assert int(ha[-1]) == 0 and int(hb[-1]) == 0
    assert torch.equal(ha, hb)
    pk, dr, _ = split_counts(hb, Z, T)
    assert np.array_equal(pk, ref["parking"]) and np.array_equal(dr, ref["driving"])
