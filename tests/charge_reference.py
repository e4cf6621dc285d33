"""The definition of include/cpm_charge.h restated twice in numpy, and a census of its branches (not a conftest: imported by
tests/test_charge.py).

Everything is derived from the oracle's state_matrix / transition_matrix (tests/side_reference.reference(..., dm=, dist=) returns them
with column 4, the driven distance, drawn: the oracle draws distances only when it is given a datamatrix, and any datamatrix will do,
because Philox stream 2 does not depend on it).  `params` is a dict: capacity_wh, power_wh, initial_wh, wh_per_km, zone_power_wh
((Z,) or None), soc_in ((C,) over the WHOLE fleet, or None); `cars` selects the cars of a shard (soc_in is sliced alike).

  charge_of       the recurrence hour by hour over all cars at once: dict(charge (Z, T) int64, used (Z, T) int64, short (Z, T) int32,
                  soc (n,) uint32, e0 (n,) int64 the initial charges).
  charge_lazy     deliberately different: car by car, a parked car is never touched and its stay is settled in closed form when it
                  next drives (k = need // P full hours, the remainder in the next, nothing after).  The same dict, plus
                  `three_phase_stays`: stays that hold full-rate hours, a remainder hour and empty hours behind it.
  census          the share of car-hours in each of six branches: short (trip not covered), covered (trip covered), full_rate (parked,
                  give == P_z > 0), remainder (0 < give < P_z), full (give == 0 < P_z), no_charger (P_z == 0).

Every comparison made with these is exact: the contract is bit-exactness."""
import numpy as np

BRANCHES = ("short", "covered", "full_rate", "remainder", "full", "no_charger")


def _setup(st, tr, Z, params, cars):
    st = np.asarray(st)[cars]
    tr = np.asarray(tr)[cars]
    n, T = st.shape
    cap = int(params["capacity_wh"])
    if params.get("soc_in") is not None:
        e0 = np.minimum(np.asarray(params["soc_in"], dtype=np.int64)[cars], cap)
    else:
        e0 = np.full(n, int(params["initial_wh"]), dtype=np.int64)
    if params.get("zone_power_wh") is not None:
        P = np.asarray(params["zone_power_wh"], dtype=np.int64)
    else:
        P = np.full(Z, int(params["power_wh"]), dtype=np.int64)
    assert e0.shape == (n,) and P.shape == (Z,)
    return st, tr, n, T, cap, e0, P, float(params["wh_per_km"])


def _trip_wh(d, wh_per_km):
    """u of the definition: rint(d * wh_per_km), round half to even; NaN or negative costs nothing"""
    with np.errstate(invalid="ignore"):
        u = np.rint(np.asarray(d, dtype=np.float64) * wh_per_km)
        return np.where(u >= 0, u, 0.0)


def _walk(st, tr, Z, params, cars):
    st, tr, n, T, cap, e0, P, whkm = _setup(st, tr, Z, params, cars)
    E = e0.copy()
    charge = np.zeros((Z, T), dtype=np.int64)
    used = np.zeros((Z, T), dtype=np.int64)
    short = np.zeros((Z, T), dtype=np.int64)
    counts = dict.fromkeys(BRANCHES, 0)
    for t in range(T):
        z = st[:, t] - 1
        drove = tr[:, t, 0] == 1
        u = _trip_wh(tr[drove, t, 3], whkm)
        Ed = E[drove]
        sh = u > Ed
        drawn = np.where(sh, Ed, np.where(sh, 0.0, u)).astype(np.int64)
        np.add.at(short, (z[drove][sh], t), 1)
        np.add.at(used, (z[drove], t), drawn)
        E[drove] = Ed - drawn
        pk = ~drove
        Pz = P[z[pk]]
        give = np.minimum(Pz, cap - E[pk])
        np.add.at(charge, (z[pk], t), give)
        E[pk] += give
        counts["short"] += int(sh.sum())
        counts["covered"] += int((~sh).sum())
        counts["full_rate"] += int(((give == Pz) & (Pz > 0)).sum())
        counts["remainder"] += int(((give > 0) & (give < Pz)).sum())
        counts["full"] += int(((give == 0) & (Pz > 0)).sum())
        counts["no_charger"] += int((Pz == 0).sum())
    assert sum(counts.values()) == n * T and E.min(initial=0) >= 0 and E.max(initial=0) <= cap
    assert short.max(initial=0) < 2 ** 31
    res = dict(charge=charge, used=used, short=short.astype(np.int32), soc=E.astype(np.uint32), e0=e0)
    return res, {k: v / max(n * T, 1) for k, v in counts.items()}


def charge_of(st, tr, Z, params, cars=slice(None)):
    return _walk(st, tr, Z, params, cars)[0]


def census(st, tr, Z, params, cars=slice(None)):
    return _walk(st, tr, Z, params, cars)[1]


def charge_lazy(st, tr, Z, params, cars=slice(None)):
    st, tr, n, T, cap, e0, P, whkm = _setup(st, tr, Z, params, cars)
    charge = np.zeros((Z, T), dtype=np.int64)
    used = np.zeros((Z, T), dtype=np.int64)
    short = np.zeros((Z, T), dtype=np.int32)
    soc = np.zeros(n, dtype=np.uint32)
    three = 0
    drove_at = tr[:, :, 0] == 1
    for i in range(n):
        E, since, zone = int(e0[i]), 0, int(st[i, 0]) - 1
        for until in list(np.flatnonzero(drove_at[i])) + [T]:
            until = int(until)
            # the stay [since, until) in `zone`, in closed form
            need, p, L = cap - E, int(P[zone]), until - since
            if p > 0 and need > 0 and L > 0:
                k, rem = divmod(need, p)
                charge[zone, since:since + min(k, L)] += p
                if k < L and rem:
                    charge[zone, since + k] += rem
                three += int(k >= 1 and rem > 0 and L > k + 1)
                E = cap if k < L else E + L * p
            if until == T:
                break
            assert int(st[i, until]) - 1 == zone                # (the trajectory is consistent)
            u = float(_trip_wh(tr[i, until, 3], whkm))
            if u > E:
                short[zone, until] += 1
                drawn = E
            else:
                drawn = int(u)
            used[zone, until] += drawn
            E -= drawn
            since, zone = until + 1, int(tr[i, until, 1]) - 1
        soc[i] = E
    return dict(charge=charge, used=used, short=short, soc=soc, e0=e0, three_phase_stays=three)


def same(a, b):
    """the four arrays of two results, exactly"""
    return all(np.array_equal(a[k], b[k]) for k in ("charge", "used", "short", "soc"))


def check_identities(res, parking, driving, params, Z):
    """the three identities of include/cpm_charge.h on a result and the counts that belong to it"""
    P = np.asarray(params["zone_power_wh"], dtype=np.int64) if params.get("zone_power_wh") is not None else np.full(Z, int(params["power_wh"]), dtype=np.int64)
    assert int(res["e0"].sum()) + int(res["charge"].sum()) - int(res["used"].sum()) == int(res["soc"].astype(np.int64).sum())
    assert (res["short"] <= driving).all() and (res["short"] >= 0).all()
    assert (res["charge"] <= P[:, None] * (parking - driving)).all() and (res["charge"] >= 0).all() and (res["used"] >= 0).all()
