"""One plain reference for every output of the fused resample (not a conftest: imported by tests/test_side_outputs.py).

`reference` runs the faithful oracle recipe -- O.initializestates -> O.solveinitialvalueproblem -> O.resampling -- and derives every
output from the oracle's state_matrix / transition_matrix by the definitions of include/*.h, in numpy:

  parking[z, t], driving[z, t]   cars with state[i, t] == z + 1 (and trans[i, t, 0] == 1), int64            (include/cpm.h)
  sum_tt_q16                     the oracle's integer sum of trans[:, :, 2]                                  (include/cpm.h)
  flows[t, o, d]                 cars with state[i, t] == o + 1, trans[i, t, 0] == 1, trans[i, t, 1] == d + 1 (include/cpm_flows.h)
  flows_csr                      the same without the zeros: np.nonzero walks the dense tensor in row-major order, so row t * Z + o
                                 holds its destinations ascending                                            (include/cpm_flows_csr.h)
  stays[t, z, L], parked[z, a]   by a walk over the hours with a `since` vector                              (include/cpm_stays.h)
  paths[t, i]                    (trans[i, t, 1] - 1) | (trans[i, t, 0] == 1) << 31                          (include/cpm_paths.h)

`check` compares one result of the product with such a reference.  Every comparison is exact: the contract is bit-exactness.
`random_tables` is the generator of tests/test_gpu_parity.py::test_randomized_small_configurations, draw for draw."""
import numpy as np

BIT = np.uint32(0x80000000)
MASK = np.uint32(0x7FFFFFFF)
KINDS = ("plain", "travel", "flows", "csr", "stays", "paths", "compat")


# ------------------------------------------------------------------------------------------------ the definitions, restated
def counts_of(st, tr, Z):
    """(parking, driving): (Z, T) int64"""
    st = np.asarray(st)
    drove = np.asarray(tr)[:, :, 0] == 1
    n, T = st.shape
    parking = np.zeros((Z, T), dtype=np.int64)
    driving = np.zeros((Z, T), dtype=np.int64)
    for t in range(T):
        parking[:, t] = np.bincount(st[:, t] - 1, minlength=Z)
        driving[:, t] = np.bincount(st[drove[:, t], t] - 1, minlength=Z)
    return parking, driving


def paths_of(st, tr):
    """(T, n) uint32 record of the matrices"""
    tr = np.asarray(tr)
    return np.ascontiguousarray(((tr[:, :, 1].astype(np.int64) - 1) | ((tr[:, :, 0] == 1).astype(np.int64) << 31)).T.astype(np.uint32))


def flows_of(st, tr, Z):
    """(T, Z, Z) int32 OD trip counts of the matrices (accumulated in int64)"""
    st = np.asarray(st)
    tr = np.asarray(tr)
    n, T = st.shape
    flows = np.zeros((T, Z, Z), dtype=np.int64)
    for t in range(T):
        drove = tr[:, t, 0] == 1
        np.add.at(flows, (t, st[drove, t] - 1, tr[drove, t, 1].astype(np.int64) - 1), 1)
    assert flows.max(initial=0) < 2 ** 31
    return flows.astype(np.int32)


def csr_of_dense(dense):
    """canonical CSR of a (T, Z, Z) tensor: dict(row_ptr (T*Z + 1,) int64, dest, count (nnz,) int32, shape)"""
    dense = np.asarray(dense)
    T, Z, _ = dense.shape
    flat = dense.reshape(T * Z, Z)
    rows, cols = np.nonzero(flat)
    row_ptr = np.zeros(T * Z + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=T * Z), out=row_ptr[1:])
    return dict(row_ptr=row_ptr, dest=cols.astype(np.int32), count=flat[rows, cols].astype(np.int32), shape=(T, Z, Z))


def stays_of(st, tr, Z):
    """(stays (T, Z, T) int32, parked (Z, T) int32) of the matrices (accumulated in int64)"""
    st = np.asarray(st)
    drove_at = np.asarray(tr)[:, :, 0] == 1
    n, T = st.shape
    since = np.zeros(n, dtype=np.int64)
    stays = np.zeros((T, Z, T), dtype=np.int64)
    for t in range(T):
        drove = drove_at[:, t]
        np.add.at(stays, (t, st[drove, t] - 1, t - since[drove]), 1)
        since[drove] = t + 1
    parked = np.zeros((Z, T), dtype=np.int64)
    still = since < T                       # (since == T: drove in hour T-1)
    np.add.at(parked, (st[still, T - 1] - 1, since[still]), 1)
    return stays.astype(np.int32), parked.astype(np.int32)


def derive(st, tr, Z):
    """every output of the matrices but the travel-time sum"""
    parking, driving = counts_of(st, tr, Z)
    flows = flows_of(st, tr, Z)
    stays, parked = stays_of(st, tr, Z)
    return dict(parking=parking, driving=driving, flows=flows, flows_csr=csr_of_dense(flows), stays=stays, parked=parked, paths=paths_of(st, tr))


def reference(O, p_drive, p_dest, Z, cpz, T, seed, *, ivp_seed=None, dm=None, dist=None):
    """The oracle's day of Z * cpz cars: the IVP with ivp_seed (default: seed), the resample with seed; with a datamatrix the
    transition matrix carries travel times and distances.  Arrays are read-only: a reference is shared and stays unchanged."""
    C = Z * cpz
    st, tr = O.initializestates(C, cpz, T)
    init = O.solveinitialvalueproblem(st, tr, p_drive, p_dest, C, Z, seed if ivp_seed is None else ivp_seed)
    st, tr = O.initializestates(C, cpz, T)
    st[:, 0] = init
    O.resampling(st, tr, C, Z, p_drive, p_dest, dm, dist, seed)
    ref = derive(st, tr, Z)
    pk, dr, _ = O.histogram(Z, st, tr)            # the oracle's own counts agree with the restatement
    assert np.array_equal(pk.astype(np.int64), ref["parking"]) and np.array_equal(dr.astype(np.int64), ref["driving"])
    ref.update(sum_tt_q16=O.sum_travel_time_q16(tr), zone0=init, state=st, trans=tr, Z=Z, cpz=cpz, T=T, seed=seed, p_drive=p_drive, p_dest=p_dest)
    for v in list(ref.values()) + list(ref["flows_csr"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------ the comparison
def _is(a, shape, dtype, order, where):
    assert isinstance(a, np.ndarray) and a.shape == tuple(shape) and a.dtype == dtype and a.flags[order + "_CONTIGUOUS"], (where, a.shape, a.dtype)


def check_csr_canonical(csr, T, Z, where=None):
    """dtypes and shapes; row_ptr starts at 0 and never falls; destinations in range, counts positive, strictly ascending in a row"""
    rp, dest, count = csr["row_ptr"], csr["dest"], csr["count"]
    assert tuple(csr["shape"]) == (T, Z, Z), where
    assert rp.dtype == np.int64 and dest.dtype == np.int32 and count.dtype == np.int32, where
    assert rp.shape == (T * Z + 1,) and rp[0] == 0 and (np.diff(rp) >= 0).all(), where
    assert dest.shape == count.shape == (int(rp[-1]),), where
    for row in np.flatnonzero(np.diff(rp) > 0):
        d = dest[rp[row]:rp[row + 1]].astype(np.int64)
        assert d[0] >= 0 and d[-1] < Z and (np.diff(d) > 0).all(), (where, int(row))
    assert (count > 0).all(), where


def check(kind, r, ref, cars=slice(None), where=None):
    """One result of the product against a reference.  kind: plain (counts), travel (counts + the travel-time sum), flows, csr,
    stays, paths, compat (want_state / want_trans: state and all four columns of trans; r["travel"] False: the step had no travel
    flag, its two travel columns are zero).  For a shard, `cars` selects the columns of paths / state that are the shard's; its
    counts, flows and stays are compared by the caller, who sums the shards."""
    assert kind in KINDS, kind
    Z, T = ref["Z"], ref["T"]
    whole = isinstance(cars, slice) and cars == slice(None)
    where = (kind, where)
    _is(r["parking"], (Z, T), np.int64, "F", where)
    _is(r["driving"], (Z, T), np.int64, "F", where)
    if whole:
        assert np.array_equal(r["parking"], ref["parking"]), where
        assert np.array_equal(r["driving"], ref["driving"]), where
    if kind == "travel" and whole:
        assert r["sum_tt_q16"] == ref["sum_tt_q16"], where
    if kind == "flows":
        _is(r["flows"], (T, Z, Z), np.int32, "C", where)
        if whole:
            assert np.array_equal(r["flows"], ref["flows"]), where
        assert np.array_equal(r["flows"].sum(axis=2, dtype=np.int64).T, r["driving"]), where
    elif kind == "csr":
        csr = r["flows_csr"]
        check_csr_canonical(csr, T, Z, where)
        if whole:
            for k in ("row_ptr", "dest", "count"):
                assert np.array_equal(csr[k], ref["flows_csr"][k]), (where, k)
    elif kind == "stays":
        _is(r["stays"], (T, Z, T), np.int32, "C", where)
        _is(r["parked"], (Z, T), np.int32, "C", where)
        if whole:
            assert np.array_equal(r["stays"], ref["stays"]), where
            assert np.array_equal(r["parked"], ref["parked"]), where
        assert np.array_equal(r["stays"].sum(axis=2, dtype=np.int64).T, r["driving"]), where
        assert np.array_equal(r["parked"].sum(axis=1, dtype=np.int64), r["parking"][:, T - 1] - r["driving"][:, T - 1]), where
    elif kind == "paths":
        want = ref["paths"][:, cars]
        _is(r["paths"], want.shape, np.uint32, "C", where)
        assert np.array_equal(r["paths"], want), where
    elif kind == "compat":
        st, tr = ref["state"][cars], ref["trans"][cars]
        if r.get("state") is not None:
            assert r["state"].dtype == np.int64 and r["state"].shape == st.shape, where
            assert np.array_equal(r["state"], st), where
        if r.get("trans") is not None:
            assert r["trans"].dtype == np.float64 and r["trans"].shape == tr.shape, where
            for k in range(4):      # (travel time and distance are drawn only by a step with the travel flag: zero otherwise)
                want = tr[:, :, k] if k < 2 or r.get("travel", True) else np.zeros_like(tr[:, :, k])
                assert np.array_equal(r["trans"][:, :, k], want), (where, k)
        assert r.get("state") is not None or r.get("trans") is not None, where


# ------------------------------------------------------------------------------------------------ random small problems
def random_tables(seed, T=None, cpz=None):
    """dict(Z, T, cpz, p_drive, p_dest) of tests/test_gpu_parity.py::test_randomized_small_configurations for `seed`: the same
    default_rng(1000 + seed) and the same order of draws.  T / cpz override what was drawn, after the draws of Z, T and cpz."""
    rng = np.random.default_rng(1000 + seed)
    Z = int(rng.integers(2, 150))
    T_drawn = int(rng.choice([1, 2, 5, 24]))
    cpz_drawn = int(rng.choice([1, 2, 7, 40, 120, 300]))
    T = T_drawn if T is None else int(T)
    cpz = cpz_drawn if cpz is None else int(cpz)
    p_drive = np.asfortranarray(rng.random((Z, T)))
    p_drive[rng.random((Z, T)) < 0.05] = 0.0
    p_drive[rng.random((Z, T)) < 0.05] = 1.0
    p_drive[rng.random((Z, T)) < 0.02] = np.nan                      # never drives (Appendix A-3)
    w = rng.random((Z, Z, T)) ** 3
    w[rng.random((Z, Z, T)) < float(rng.choice([0.0, 0.5, 0.9]))] = 0.0  # sparse rows
    w[:, rng.random(Z) < 0.1, :] = 0.0                               # zones nobody drives to
    for o in np.flatnonzero(rng.random(Z) < 0.1):                    # single-destination rows
        w[o, :, :] = 0.0
        w[o, int(rng.integers(0, Z)), :] = 1.0
    w[rng.random(Z) < 0.1, :, :] = 0.0                               # all-zero rows: destination = origin, counted as driving
    p_dest = np.zeros((Z, Z, T), order="F")
    for t in range(T):
        for o in range(Z):
            tot = 0.0
            for v in w[o, :, t]:
                tot += v                                             # the sequential sum of src/createpdestin.jl:31-35
            if tot > 0:
                p_dest[o, :, t] = w[o, :, t] / tot
    return dict(Z=Z, T=T, cpz=cpz, p_drive=p_drive, p_dest=p_dest)
