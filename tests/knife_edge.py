"""Days whose draws land exactly ON a table edge, or one step (2^-53) beside it (not a conftest: imported by tests/test_knife_edge.py).

The sampler makes two comparisons, and the reference writes both with `<=`: `RndVar <= p_drive[origin, t]` (src/resampling.jl:15) and
`range_low < RndVar <= range_up` (:40).  On random tables a 53-bit draw meets an edge with probability 2^-53, so no parity test on
random tables can tell `<=` from `<`.  Philox is counter-based: the draws of car g at step s are known before the run
(O.uniforms(seed, g, s, 0) = (u0, u1); kb = u0 * 2^53 decides the drive, kc = u1 * 2^53 the destination, both exact integers).  The
tables of these days are built around them.

INTEGER TABLES.  Every entry of p_drive and p_dest is m * 2^-53 with m an integer, and every p_dest row has sum(m) <= 2^53.  Every
partial sum of a row is then an exact double whatever the order of summation -- the oracle's sequential CDF, Julia's pairwise sum and
the device's checkpointed running sums agree exactly -- and floor(p * 2^53) is m itself.  The builder checks both (the float tables
times 2^53 are the integer ones; O.build_cdf equals the integer cumulative sums times 2^-53).

CAUSAL PLANTING.  Hour t reads column t of both tables, and who stands in a zone at hour t depends on the columns before t only.  So
the day is built hour by hour with the stepper below (the oracle's rule in integers, D1 and the u == 0 case included).  At hour t,
in every zone z that holds at least 4 cars:
  Bernoulli    one car a of the zone; p_drive[z, t] = kb_a * 2^-53 ((z + t) even: u == p, a DRIVES) or (kb_a - 1) * 2^-53 ((z + t) odd: u is one
               step above p, a must NOT drive).
  categorical  when the zone has at least 3 drivers under the p_drive just fixed: up to 6 of them with ascending draws more than 2 apart,
               spread over the zone's drivers, the largest draw among them, each with a destination slot of its own; the slots of a row are at least 3 apart, so the two zones behind each slot hold
               no weight.  Plant 0, 2, 4 (counted from 0): the running sum at the slot is exactly kc -- the destination is the slot (ON
               the breakpoint).  Plant 1, 3, 5: the running sum is kc - 1 -- the destination is the next zone that holds weight, the
               next plant's slot, across at least two zero-weight zones (AFTER the breakpoint; the high 32 bits of such a draw equal
               those of a CDF entry, which is what sends a real car of a real launch through the tie fallback).  Rows with
               (z + t) % 3 != 0 give zone Z - 1 the remainder up to exactly 2^53; the others stop at the last plant with a total
               below 1: an even last plant sits exactly ON THE TOTAL (the D1 clamp boundary), an odd one is one step above it and
               FALLS THROUGH to the last zone with weight, its own slot.
A zone with fewer cars keeps its background column: 12 random integer cells per row that sum to 2^53, p_drive in [0.25, 0.75).

The expected outcome of a plant follows from the construction and the reference's comparison alone; it is written down before the
stepper runs the hour.  Expected destinations are 0-based, like the per-car record of resample(paths=True).

TWO KINDS OF DAY.  Column t serves IVP hour t and resample hour t alike, so a plant made for the resample would change the IVP in front
of it.  A RESAMPLE day skips the IVP: the start is installed with set_state, columns 0 .. T-1 are planted for steps T-1 .. 2T-2 (the
last column is sampled and never applied).  An IVP day plants columns 0 .. T-2 for steps 0 .. T-2.
"""
import numpy as np

ONE = 1 << 53
STEP = 2.0 ** -53

DRIVES, STAYS, ON_BREAK, AFTER_BREAK, ON_TOTAL, FALLS = "drives", "must not drive", "on the breakpoint", "after the breakpoint", "on the total", "falls through"
KINDS = (DRIVES, STAYS, ON_BREAK, AFTER_BREAK, ON_TOTAL, FALLS)
# conditions, not measurements: what a resample day of Z x 40 cars must plant at least (a seed that misses one is changed, never the floor)
FLOORS = {DRIVES: 200, STAYS: 200, ON_BREAK: 1000, AFTER_BREAK: 800, ON_TOTAL: 25, FALLS: 80}
MUTANTS = ("bernoulli <", "categorical <", "categorical on the high 32 bits")

_MIN_CARS, _MIN_DRIVERS, _MAX_PLANTS, _BACKGROUND_CELLS = 4, 3, 6, 12


def draws(O, seed, cars, steps):
    """(kb, kc): int64 arrays (len(cars), len(steps)) of the 53-bit draws of the global cars `cars` at the Philox steps `steps`."""
    import ctypes as C
    fn = O.lib().orc_uniforms
    a, b = C.c_double(), C.c_double()
    pa, pb = C.byref(a), C.byref(b)
    kb = np.empty((len(cars), len(steps)), dtype=np.int64)
    kc = np.empty_like(kb)
    for i, g in enumerate(cars):
        g = int(g)
        for j, s in enumerate(steps):
            fn(seed, g, int(s), 0, pa, pb)
            kb[i, j] = int(a.value * ONE)       # exact: u is a 53-bit integer times 2^-53
            kc[i, j] = int(b.value * ONE)
    return kb, kc


def categorical(row, k, mutant=None):
    """0-based destinations of the draws k (int64 array) on the integer row `row` (which holds weight): first j with range_low < u <=
    range_up, D1 beside it (above the total: the last zone with weight; u == 0: the first)."""
    S = np.cumsum(row)
    weight = np.nonzero(row > 0)[0]
    if mutant == MUTANTS[1]:
        j = np.searchsorted(S, k, side="right")                                 # first j with u < cdf[j]
    elif mutant == MUTANTS[2]:
        j = np.searchsorted(S >> 21, k >> 21, side="left")                      # first j with hi32(u) <= hi32(cdf[j])
    else:
        j = np.searchsorted(S, k, side="left")                                  # first j with u <= cdf[j] (range_low < u: u > 0)
    j = np.where(j >= row.shape[0], weight[-1], j)
    return np.where(k == 0, weight[0], j)


def hour(zone, kb, kc, m_drive_col, m_dest_col, mutant=None):
    """One hour of the reference's rule in integers: zone (n,) 1-based, the hour's draws, column t of the integer tables ((Z,) and (Z, Z)
    [origin, destination]).  Returns (drove bool (n,), destination (n,) 1-based; the own zone of a car that did not drive).
    mutant: one of MUTANTS -- the wrong comparison a kernel could make."""
    thr = m_drive_col[zone - 1]
    drove = kb < thr if mutant == MUTANTS[0] else kb <= thr                     # RndVar <= driving_probability
    dest = zone.copy()
    for z in np.unique(zone[drove]):
        sel = np.nonzero(drove & (zone == z))[0]
        row = m_dest_col[z - 1]
        if row.sum() == 0:                                                      # an all-zero row: the destination is the origin
            continue
        dest[sel] = categorical(row, kc[sel], mutant) + 1
    return drove, dest


def run(day, mutant=None):
    """The whole day on its finished tables: dict(state (n, T) 1-based zones -- of an IVP day: column T-1 is the post-IVP state --,
    drove (n, hours) bool, dest (n, hours) 1-based, parking, driving (Z, hours) int64)."""
    Z, T, n, hours = day["Z"], day["T"], day["n"], day["hours"]
    state = np.zeros((n, T), dtype=np.int64)
    drove = np.zeros((n, hours), dtype=bool)
    dest = np.zeros((n, hours), dtype=np.int64)
    state[:, 0] = day["zone0"]
    for t in range(hours):
        drove[:, t], dest[:, t] = hour(state[:, t], day["kb"][:, t], day["kc"][:, t], day["m_drive"][:, t], day["m_dest"][:, :, t], mutant)
        if t + 1 < T:
            state[:, t + 1] = dest[:, t]
    parking = np.stack([np.bincount(state[:, t] - 1, minlength=Z) for t in range(hours)], axis=1).astype(np.int64)
    driving = np.stack([np.bincount(state[drove[:, t], t] - 1, minlength=Z) for t in range(hours)], axis=1).astype(np.int64)
    return dict(state=state, drove=drove, dest=dest, parking=parking, driving=driving)


def _background(Z, T, rng):
    m_drive = rng.integers(ONE // 4, 3 * (ONE // 4), size=(Z, T), dtype=np.int64)
    m_dest = np.zeros((Z, Z, T), dtype=np.int64)
    cells = min(_BACKGROUND_CELLS, Z)
    for t in range(T):
        for z in range(Z):
            cuts = np.unique(rng.integers(1, ONE, size=cells - 1, dtype=np.int64))
            assert cuts.shape[0] == cells - 1
            m_dest[z, rng.choice(Z, size=cells, replace=False), t] = np.diff(np.concatenate([[0], cuts, [ONE]]))
    return m_drive, m_dest


def _forced_slots(Z):
    """slots some rows must use: 0, the edges of the 32- and 64-entry pieces of a row, the first and the last zone of a destination
    group (ceil(Z / 32) consecutive zones); None: no slot forced"""
    G = -(-Z // 32)
    want = [0, 31, 32, 63, 64, 5 * G, 6 * G - 1, None, None, None]
    return [s for s in want if s is None or s <= Z - 4], G


def build_day(O, Z, T, zone0, cars, seed, kind="resample", table_seed=1, floor_scale=1.0, max_car=None):
    """The day of the global cars `cars` (ids, in the context's order) that start in the 1-based zones `zone0`.  kind "resample" or
    "ivp".  floor_scale: FLOORS times this must be planted (None: waived -- tiny days); max_car: no planted car's id may exceed it."""
    assert kind in ("resample", "ivp")
    cars = np.asarray(cars, dtype=np.uint64)
    zone0 = np.asarray(zone0, dtype=np.int64)
    n = cars.shape[0]
    hours = T if kind == "resample" else T - 1
    steps = np.arange(hours) + (T - 1 if kind == "resample" else 0)
    kb, kc = draws(O, seed, cars, steps)
    rng = np.random.default_rng(table_seed)
    m_drive, m_dest = _background(Z, T, rng)
    forced, G = _forced_slots(Z)
    plants = []                                  # (hour 0-based, car index in the context, kind, expected: 1 / 0 or the 0-based destination)
    rows = 0
    zone = zone0.copy()
    for t in range(hours):
        order = np.argsort(zone, kind="stable")
        bounds = np.searchsorted(zone[order], np.arange(1, Z + 2))
        for z in range(Z):
            idx = order[bounds[z]:bounds[z + 1]]
            if idx.shape[0] < _MIN_CARS:
                continue
            # ---- Bernoulli: the car at the upper quartile of the zone's draws (so that most of the zone drives)
            a = idx[np.argsort(kb[idx, t], kind="stable")[(3 * idx.shape[0]) // 4]]
            if (z + t) % 2 == 0 or kb[a, t] == 0:
                m_drive[z, t] = kb[a, t]
                plants.append((t, int(a), DRIVES, 1))
            else:
                m_drive[z, t] = kb[a, t] - 1
                plants.append((t, int(a), STAYS, 0))
            # ---- categorical
            drivers = idx[kb[idx, t] <= m_drive[z, t]]
            drivers = drivers[np.argsort(kc[drivers, t], kind="stable")]
            keep = []
            for d in drivers:
                if kc[d, t] - (kc[keep[-1], t] if keep else -2) > 2:     # (the first: kc >= 1, so that its slot holds weight)
                    keep.append(d)
            if len(keep) < _MIN_DRIVERS:
                continue
            keep = np.asarray(keep)
            # (half of the rows that stop at their last plant take 5 plants at the most: an even last plant, ON the total)
            most = min(_MAX_PLANTS - ((z + t) % 6 == 0), keep.shape[0])
            keep = keep[np.unique(np.rint(np.linspace(0, keep.shape[0] - 1, most)).astype(np.int64))]
            force = forced[rows % len(forced)]
            rows += 1
            klass = int(rng.integers(3)) if force is None else force % 3
            pool = np.arange(klass, Z - 3, 3)
            pool = pool[pool != force] if force is not None else pool
            slots = rng.choice(pool, size=keep.shape[0] - (force is not None), replace=False)
            slots = np.sort(np.concatenate([slots, [force]]) if force is not None else slots).astype(np.int64)
            remainder = (z + t) % 3 != 0
            m_dest[z, :, t] = 0
            running = 0
            for i, (car, slot) in enumerate(zip(keep, slots)):
                k = int(kc[car, t])
                last = i == keep.shape[0] - 1
                edge = k if i % 2 == 0 else k - 1
                m_dest[z, slot, t] = edge - running
                running = edge
                if i % 2 == 0:
                    plants.append((t, int(car), ON_TOTAL if last and not remainder else ON_BREAK, int(slot)))
                elif not last:
                    plants.append((t, int(car), AFTER_BREAK, int(slots[i + 1])))
                elif remainder:
                    plants.append((t, int(car), AFTER_BREAK, Z - 1))
                else:
                    plants.append((t, int(car), FALLS, int(slot)))
            if remainder:
                m_dest[z, Z - 1, t] = ONE - running
        _, dest = hour(zone, kb[:, t], kc[:, t], m_drive[:, t], m_dest[:, :, t])
        if t + 1 < T:
            zone = dest
    p_drive = np.asfortranarray(m_drive.astype(np.float64) * STEP)
    p_dest = np.asfortranarray(m_dest.astype(np.float64) * STEP)
    day = dict(Z=Z, T=T, n=n, hours=hours, kind=kind, seed=seed, cars=cars, zone0=zone0, steps=steps, kb=kb, kc=kc, m_drive=m_drive, m_dest=m_dest,
               p_drive=p_drive, p_dest=p_dest, plants=plants, group=G)
    day["counts"] = {k: sum(1 for p in plants if p[2] == k) for k in KINDS}
    _check_day(O, day, floor_scale, max_car)
    for v in day.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return day


def _check_day(O, day, floor_scale, max_car):
    Z, T, m_drive, m_dest = day["Z"], day["T"], day["m_drive"], day["m_dest"]
    assert (m_drive >= 0).all() and (m_drive <= ONE).all() and (m_dest >= 0).all() and (m_dest.sum(axis=1) <= ONE).all()
    # the float tables ARE the integer ones, and every running sum of a row is exact in the oracle's order of summation
    assert np.array_equal(day["p_drive"] * float(ONE), m_drive.astype(np.float64)) and np.array_equal((day["p_drive"] * float(ONE)).astype(np.int64), m_drive)
    assert np.array_equal((day["p_dest"] * float(ONE)).astype(np.int64), m_dest)
    sums = np.cumsum(m_dest, axis=1).transpose(2, 0, 1)                          # [t][o][d]
    assert np.array_equal(O.build_cdf(day["p_dest"]), sums.astype(np.float64) * STEP)
    assert np.array_equal((O.build_cdf(day["p_dest"]) * float(ONE)).astype(np.int64), sums)
    # one plant per (hour, car, comparison)
    assert len({(t, c, k in (DRIVES, STAYS)) for t, c, k, _ in day["plants"]}) == len(day["plants"])
    if floor_scale is not None:
        for k in KINDS:
            assert day["counts"][k] >= FLOORS[k] * floor_scale, (k, day["counts"], floor_scale)
        slots = {e for _, _, k, e in day["plants"] if k not in (DRIVES, STAYS)}       # the destinations the planted cars reach
        G = day["group"]
        for s in (0, 31, 32, 63, 64):
            assert s > Z - 4 or s in slots, s
        assert any(s % G == 0 for s in slots) and any(s % G == G - 1 for s in slots)
    if max_car is not None:
        assert max(int(day["cars"][c]) for _, c, _, _ in day["plants"]) <= max_car


def plants_hold(day, drove, dest0):
    """The plants against an outcome: drove (n, hours) bool, dest0 (n, hours) 0-based destinations.  Returns the plants that do NOT hold."""
    bad = []
    for t, c, k, e in day["plants"]:
        if k in (DRIVES, STAYS):
            ok = bool(drove[c, t]) == bool(e)
        else:
            ok = bool(drove[c, t]) and int(dest0[c, t]) == e
        if not ok:
            bad.append((t, c, k, e, bool(drove[c, t]), int(dest0[c, t])))
    return bad


def flipped_p_drive(day):
    """p_drive with every planted zone-hour moved one step the other way: where a car DRIVES on the edge the edge goes down by 2^-53,
    where a car must NOT drive it goes up -- every Bernoulli plant flips at the hour it was planted for."""
    m = day["m_drive"].copy()
    state = run(day)["state"]
    for t, c, k, _ in day["plants"]:
        if k == DRIVES:
            m[state[c, t] - 1, t] -= 1
        elif k == STAYS:
            m[state[c, t] - 1, t] += 1
    assert (m >= 0).all() and (np.abs(m - day["m_drive"]) <= 1).all()
    return np.asfortranarray(m.astype(np.float64) * STEP)
