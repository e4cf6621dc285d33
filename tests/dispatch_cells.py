"""The grouped path's dispatch, restated: which INSTANTIATION of its hourly kernels a problem runs (not a conftest, no GPU).

Every hourly launcher of csrc/cpm_grouped.h, cpm_day.h, cpm_count.h and cpm_batch.h is a ladder over template parameters (CPT cars
per thread, NQ LDS-DMA instructions per wave for the row pack, GROUPED / SPARSE / PERM), and each rung is separately compiled code.
This module restates the host rules that choose the rung (csrc/cpm_dispatch.h: the rules and each family's tables, walked by
cell_walk) -- from the problem's Z, its cars and the context's options -- and derives from them

  reachable()    every cell a problem that fits the grouped path can launch, per launcher,
  unreachable()  the instantiations the build compiles that no such problem can launch, each with the rule that excludes it,
  CASES          the case table of tests/test_dispatch_cells.py: one problem per reachable cell, on the edges of the rules,
  predict()      the launch record (Sampler.last_step()["cells"], CPM_INFO_CELL_* of include/cpm.h) a step of a case must leave.

The record is written by each family's launch body (grouped_launch_sample_t and its like) from its own template parameters, so a
disagreement between predict() and the record is a finding about a ladder or about this restatement; tests/test_dispatch_cells.py
(CPU part) checks the band edges, that CASES covers reachable() entirely, that every case fits, and -- through tests/dispatch_probe.cc,
a host program over cpm_dispatch.h -- that the rules restated here are the library's for every Z and every mean.
"""
import functools
from collections import namedtuple

# ------------------------------------------------------------------------------------------------ constants (csrc/cpm_grouped.h)
K_GROUPS = 32
SAMPLE_BLOCK = 256
MAX_ZONES_PER_GROUP = 1024          # kMaxZonesPerGroup: LDS bins of the placing kernel
FUSED_ZPG = 256                     # kFusedZpg
HEAVY = 4                           # kHeavy
CNT_XCC_SHIFT = 26                  # kCntXccShift (the day launch keeps its bucket regions below it)

# record coding (include/cpm.h)
SAMPLE, HOUR, HOUR_PF, DAY, HEAVY_K, COUNT, PLACE, BATCH_SAMPLE, BATCH_PLACE, BATCH_COUNT = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
F_GROUPED, F_SPARSE, F_PERM = 1, 2, 4
KIND_NAMES = {SAMPLE: "sample", HOUR: "hour", HOUR_PF: "hour_pf", DAY: "day", HEAVY_K: "heavy", COUNT: "count", PLACE: "place",
              BATCH_SAMPLE: "batch_sample", BATCH_PLACE: "batch_place", BATCH_COUNT: "batch_count"}


def word(kind, cpt, nq=0, grouped=False, sparse=False, perm=False):
    return kind | cpt << 8 | nq << 16 | ((F_GROUPED if grouped else 0) | (F_SPARSE if sparse else 0) | (F_PERM if perm else 0)) << 24


def place_word(pb, kruns, batch=False):
    return (BATCH_PLACE if batch else PLACE) | kruns << 8 | (pb // 64) << 16


def describe(w):
    if w == 0:
        return "none"
    kind, a, b, fl = w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24
    if kind in (PLACE, BATCH_PLACE):
        return f"{KIND_NAMES[kind]}<PB {b * 64}, KRUNS {a}>"
    flags = "".join(n for bit, n in ((F_GROUPED, " GROUPED"), (F_SPARSE, " SPARSE"), (F_PERM, " PERM")) if fl & bit)
    return f"{KIND_NAMES.get(kind, kind)}<CPT {a}, NQ {b}{flags}>"


# ------------------------------------------------------------------------------------------------ row packs
def pack_guide_bits(Z):
    g = 3
    while (1 << g) < Z:
        g += 1
    return max(3, g - 2)


def pack_zq(Z):
    return (Z + 31 + 31) // 32 * 32


def pack_guide_words(G):
    return (1 << G) // 2 + 4


def pack_row_words(Zq, G, smap=0):
    return max(256, pack_guide_words(G) + Zq + (Zq // 2 if smap else 0))


def pack_row_fits(Z):
    return 2 <= Z <= 32768 and 4 * pack_row_words(pack_zq(Z), pack_guide_bits(Z)) <= 150 * 1024


def need_of(Z):
    """16-byte pieces of a dense row pack over the 256 lanes of a sampler workgroup: LDS-DMA instructions per wave"""
    return (pack_row_words(pack_zq(Z), pack_guide_bits(Z)) // 4 + SAMPLE_BLOCK - 1) // SAMPLE_BLOCK


# need -> NQ: the ladders differ (SampleCells, HourCells, HourPfCells, DayCells, HeavyCells of csrc/cpm_dispatch.h)
LADDERS = {SAMPLE: (1, 2, 3, 4, 5, 6, 8, 12, 20, 40), HOUR: (1, 2, 3, 4, 5, 6, 8, 12), HOUR_PF: (1, 2, 3, 4, 5, 6, 8, 12),
           DAY: (1, 2, 3, 4, 5, 6, 8, 12), HEAVY_K: (2, 5, 12, 40)}
SPARSE_NQ = {SAMPLE: 1, HOUR: 1, HOUR_PF: 1, DAY: 1, HEAVY_K: 2}   # a sparse pack is one LDS-DMA instruction per wave


def ladder_nq(kind, need):
    for nq in LADDERS[kind]:
        if need <= nq:
            return nq
    return LADDERS[kind][-1]


# ------------------------------------------------------------------------------------------------ cars per thread
def cpt_narrow(mean):
    """grouped_cpt: the sampler once a heavy bucket was seen, and the pf / day / heavy launchers"""
    return 1 if mean <= 224 else (2 if mean <= 560 else 4)


def cpt_wide(mean):
    """grouped_cpt_wide: the sampler, the count-only kernel and the one-launch hour while no heavy bucket was seen; the batched sampler"""
    return 1 if mean <= 170 else (2 if mean <= 340 else (4 if mean <= 700 else 6))


WIDE_EDGES = {1: 170, 2: 340, 4: 700, 6: 701}     # the fullest workgroup of every CPT (6: the first mean that takes it)
NARROW_EDGES = {1: 224, 2: 560, 4: 561}
WIDE_FROM = {1: 1, 2: 171, 4: 341, 6: 701}        # the smallest mean of every CPT
NARROW_FROM = {1: 1, 2: 225, 4: 561}


def mean_of(n, Z):
    return (n + Z - 1) // Z


# ------------------------------------------------------------------------------------------------ groups, placing, fit
def zpg_of(Z, general=False):
    if general:
        return max(1, (Z + K_GROUPS - 1) // K_GROUPS)
    s = 0
    while (K_GROUPS << s) < Z:
        s += 1
    return 1 << s


def idbits(Z, general=False):
    b = 1
    while (1 << b) < zpg_of(Z, general):
        b += 1
    return 32 - b


PlaceShape = namedtuple("PlaceShape", "pb kruns bpg")


def place_shape(Z):
    pb = 512 if zpg_of(Z) <= 512 else 1024
    seg = pb // 16
    bpg = 8 if Z < 1024 else 16
    while bpg < 128 and (Z + bpg - 1) // bpg > 4 * seg:
        bpg *= 2
    kruns = 4 if (Z + bpg - 1) // bpg <= 4 * seg else 8
    return PlaceShape(pb, kruns, bpg)


def place_shape_fits(Z):
    p = place_shape(Z)
    return (Z + p.bpg - 1) // p.bpg <= 8 * (p.pb // 16)


def grouped_cap(n, Z, cap_mult=4):
    return (max(cap_mult * mean_of(n, Z), 1024) + 63) // 64 * 64


def odd_lines(words):
    return words + 32 if (words // 32) % 2 == 0 else words


def grouped_scap(cap):
    return odd_lines((max(64, cap // 4) + 31) // 32 * 32)


def grouped_path_fits(n, Z, cap_mult=4):
    """grouped_path_fits: the row pack fits LDS, ids fit the packed driver word, n < 2^30, the bucket and run arrays fit their budget"""
    if not pack_row_fits(Z) or n < 1 or n >= 1 << 30:
        return False
    cap = grouped_cap(n, Z, cap_mult)
    if n > 1 << idbits(Z) or zpg_of(Z) > MAX_ZONES_PER_GROUP:
        return False
    if not place_shape_fits(Z):
        return False
    nbytes = Z * cap * 4 * 3 + 2 * Z * K_GROUPS * grouped_scap(cap) * 4
    return nbytes <= (24 if cap_mult <= 4 else 80) << 30


def fused_shape_ok(Z, sparse=False):
    """an instantiation of the one-launch forms exists (the rule reads the power-of-two groups whatever the pack; a sparse pack, at
    most 512 cells, is one instruction per wave)"""
    if sparse:
        return zpg_of(Z) <= FUSED_ZPG
    return zpg_of(Z) <= FUSED_ZPG and need_of(Z) <= 12


def heavy_threshold(cpt):
    """a bucket is heavy above kHeavy x the slots of its sampler workgroup (at most four cars per lane count)"""
    return HEAVY * min(cpt, 4) * SAMPLE_BLOCK


def cap_mult_for(largest_bucket, n, Z):
    """the bucket regions after the library grew them (doubling from 4 x the mean) until `largest_bucket` cars fit one"""
    cm = 4
    while grouped_cap(n, Z, cm) < largest_bucket:
        cm *= 2
    return cm


# ------------------------------------------------------------------------------------------------ bands
@functools.lru_cache(maxsize=None)
def nq_bands():
    """{NQ of the sampler ladder: (first Z, last Z)} over every Z whose dense row pack fits"""
    bands = {}
    for Z in range(2, 32769):
        if not pack_row_fits(Z):
            continue
        nq = ladder_nq(SAMPLE, need_of(Z))
        lo, hi = bands.get(nq, (Z, Z))
        bands[nq] = (min(lo, Z), max(hi, Z))
    return bands


def fused_last_z():
    return max(Z for Z in range(2, 32769) if pack_row_fits(Z) and fused_shape_ok(Z))


# ------------------------------------------------------------------------------------------------ what a step launches
def predict(Z, n, T, *, step, fused=0, parts=1, sparse=False, last_hour=1, zone_order=2, perm_valid=False):
    """The launch record of one grouped step (grouped_run, restated): step "ivp" (T - 1 applied hours) or "resample" (T - 1 applied
    hours and hour T, which is sampled and never applied), without travel times or side outputs.  fused: CPM_OPT_FUSED (0, 1, 3, 6,
    8); parts: CPM_INFO_PARTS going in; last_hour: CPM_OPT_LAST_HOUR; zone_order: CPM_OPT_ZONE_ORDER; perm_valid: an IVP has run in
    this context.  -> dict(applied, heavy, last, place, batch) of record words."""
    ivp = step == "ivp"
    mean = mean_of(n, Z)
    heavy_seen = parts > 1
    need = 1 if sparse else need_of(Z)

    def nq(kind):
        return SPARSE_NQ[kind] if sparse else ladder_nq(kind, need)

    cpt_s = cpt_narrow(mean) if heavy_seen else cpt_wide(mean)      # grouped_launch_sample / _count
    rec = dict(applied=0, heavy=0, last=0, place=0, batch=0)
    hours = T - 1 if ivp else T
    shape = fused != 0 and not heavy_seen and fused_shape_ok(Z, sparse)
    day_n = 0
    if shape and fused >= 6 and grouped_cap(n, Z) < 1 << CNT_XCC_SHIFT:
        day_n = hours if ivp else hours - 1
    if day_n < 2:
        day_n = 0
    cap = grouped_cap(n, Z)
    permute = (zone_order == 1 or (zone_order == 2 and sparse)) and perm_valid and Z * K_GROUPS * grouped_scap(cap) * 4 < 1 << 32
    p = place_shape(Z)
    pending = False
    if day_n:
        rec["applied"] = word(DAY, cpt_narrow(mean), nq(DAY), True, sparse)
        pending = True
    for t in range(day_n, hours):
        last = (not ivp) and t + 1 == T
        grouped = (not last) or heavy_seen
        after_day = day_n > 0 and t == day_n
        pf = shape and (fused in (3, 4) or after_day)
        fuse = grouped and not last and shape and not pf
        role = "last" if last else "applied"
        if not pf and pending:
            rec["place"] = place_word(p.pb, p.kruns)
            pending = False
        if pf:
            rec[role] = word(HOUR_PF, cpt_narrow(mean), nq(HOUR_PF), grouped, sparse)
            pending = False
        elif fuse:
            rec[role] = word(HOUR, cpt_wide(mean), nq(HOUR), True, sparse, permute and t < T - 1)
        elif grouped:
            rec[role] = word(SAMPLE, cpt_s, nq(SAMPLE), True, sparse)
        elif last_hour:
            rec[role] = word(COUNT, cpt_s, 0, False, sparse)
        else:
            rec[role] = word(SAMPLE, cpt_s, nq(SAMPLE), False, sparse)
        if grouped and not fuse and not pf and heavy_seen:
            rec["heavy"] = word(HEAVY_K, cpt_narrow(mean), nq(HEAVY_K), True, sparse)
        if not last:
            if pf:
                pending = True
            elif not fuse:
                rec["place"] = place_word(p.pb, p.kruns)
    if pending:
        rec["place"] = place_word(p.pb, p.kruns)
    return rec


def predict_batch(Z, n, T, *, sparse=False, last_hour=1):
    """batch_run, restated (no travel times): the batched sampler with the wide rule, hour T counts only or in the plain form"""
    cpt = cpt_wide(mean_of(n, Z))
    p = place_shape(Z)
    return dict(applied=0, heavy=0, batch=word(BATCH_SAMPLE, cpt, 0, True, sparse) if T >= 2 else 0,
                last=word(BATCH_COUNT, cpt, 0, False, sparse) if last_hour else word(BATCH_SAMPLE, cpt, 0, False, sparse),
                place=place_word(p.pb, p.kruns, batch=True) if T >= 2 else 0)


# ------------------------------------------------------------------------------------------------ the template grids the build compiles
def template_grid():
    """every instantiation the launchers name (record words)"""
    g = set()
    for grouped in (False, True):
        for cpt in (1, 2, 4, 6):
            g |= {word(SAMPLE, cpt, nq, grouped) for nq in LADDERS[SAMPLE]} | {word(SAMPLE, cpt, 1, grouped, True)}
            g |= {word(BATCH_SAMPLE, cpt, 0, grouped, sp) for sp in (False, True)}
        for cpt in (1, 2, 4):
            g |= {word(HOUR_PF, cpt, nq, grouped) for nq in LADDERS[HOUR_PF]} | {word(HOUR_PF, cpt, 1, grouped, True)}
    for cpt in (1, 2, 4, 6):
        for perm in (False, True):
            g |= {word(HOUR, cpt, nq, True, False, perm) for nq in LADDERS[HOUR]} | {word(HOUR, cpt, 1, True, True, perm)}
        g |= {word(COUNT, cpt, 0, False, sp) for sp in (False, True)} | {word(BATCH_COUNT, cpt, 0, False, sp) for sp in (False, True)}
    for cpt in (1, 2, 4):
        g |= {word(DAY, cpt, nq, True) for nq in LADDERS[DAY]} | {word(DAY, cpt, 1, True, True)}
        g |= {word(HEAVY_K, cpt, nq, True) for nq in LADDERS[HEAVY_K]} | {word(HEAVY_K, cpt, 2, True, True)}
    for pb in (512, 1024):
        for kruns in (4, 8):
            g |= {place_word(pb, kruns), place_word(pb, kruns, batch=True)}
    return g


SPARSE_Z = 700   # the sparse cells are asked of one table shape (tests/test_sparse_upload.py); any Z reaches the same cells


@functools.lru_cache(maxsize=None)
def reachable():
    """Every cell some problem that fits the grouped path launches: each Z whose pack fits, at the smallest mean of every CPT of both
    rules (where that many cars still fit), through every step, form, heavy state and option."""
    cells = set()
    means = sorted(set(WIDE_FROM.values()) | set(NARROW_FROM.values()))
    seen = set()
    for Z in range(2, 32769):
        if not pack_row_fits(Z):
            continue
        for sparse in ((False, True) if Z == SPARSE_Z else (False,)):
            for mean in means:
                n = Z * mean
                if not grouped_path_fits(n, Z):
                    continue
                key = (need_of(Z), mean, place_shape(Z)[:2], fused_shape_ok(Z, sparse), sparse)
                if key in seen:
                    continue
                seen.add(key)
                for fused in (0, 1, 3, 6):
                    for parts in (1, 2):
                        for perm in (False, True):
                            for lh in (0, 1):
                                for step in ("ivp", "resample"):
                                    r = predict(Z, n, 3, step=step, fused=fused, parts=parts, sparse=sparse, last_hour=lh,
                                                zone_order=1 if perm else 0, perm_valid=perm)
                                    cells |= {w for w in r.values() if w}
                for lh in (0, 1):
                    cells |= {w for w in predict_batch(Z, n, 3, sparse=sparse, last_hour=lh).values() if w}
    return frozenset(cells)


def unreachable():
    """{instantiation: the rule that excludes it}"""
    out = {}
    for w in sorted(template_grid() - reachable()):
        kind, a, b = w & 255, (w >> 8) & 255, (w >> 16) & 255
        if kind in (PLACE, BATCH_PLACE):
            out[w] = ("KRUNS = 8 needs more than 4 x PB / 16 zones per placing block at 128 blocks per group: Z > 16,384 at PB = 512, where "
                      "zones per group exceed 512 and PB is 1,024; Z > 32,768 at PB = 1,024, which pack_row_fits refuses")
        elif kind == SAMPLE and b == 40:
            out[w] = ("NQ = 40 begins at Z = 16,385: 1,024 zones per group leave 22 id bits, n <= 2^22, a mean bucket <= 255, "
                      f"so CPT {a} (mean > {WIDE_FROM[a] - 1}) cannot be chosen")
        else:
            out[w] = "no rule found: resolve against the C++"
    return out


# ------------------------------------------------------------------------------------------------ the case table
# table: "synth" the oracle's / the library's flat synthetic tables; "hot" a hand-made table that sends a fixed share of every hour's
# drivers to one zone (heavy buckets); "sparse" the Z = 700 datamatrix of tests/test_sparse_upload.py, uploaded under
# CPM_OPT_SPARSE_UPLOAD.  kind: "hourly" an IVP and resamples under CPM_OPT_FUSED `fused`; "heavy"; "batch" two fleets.
Case = namedtuple("Case", "id Z T cpz table kind fused perm")


def _t_of(Z):
    return 3 if Z <= 8192 else 2


def _cases():
    bands = nq_bands()
    out = []

    def add(tag, Z, cpz, table="synth", kind="hourly", fused=0, perm=False):
        out.append(Case(f"{tag}-Z{Z}x{cpz}", Z, _t_of(Z), cpz, table, kind, fused, perm))

    # two launches per hour: every (CPT, NQ) of k_grouped_sample, grouped and (hour T) plain, and the count-only kernel's cpt
    for nq, (lo, hi) in sorted(bands.items()):
        for cpt, cpz in WIDE_EDGES.items():
            if nq == 40:
                cpz = {1: 170, 2: 255}.get(cpt)          # (n <= 2^22)
                if cpz is None:
                    continue
            add(f"two-nq{nq}-cpt{cpt}", lo, cpz)
        if nq <= 20:
            add(f"two-nq{nq}-top", hi, 40)               # the band's upper edge, cheaply
    # one launch per hour: every (CPT, NQ <= 12), each with the zones in zone order and dealt largest-first (PERM)
    for nq, (lo, hi) in sorted(bands.items()):
        if nq > 12:
            continue
        for cpt, cpz in WIDE_EDGES.items():
            add(f"one-nq{nq}-cpt{cpt}", lo, cpz, fused=1, perm=True)
    # the heavy kernel: {1, 2, 4} x {2, 5, 12, 40}  (need 1, 3, 5, 6 and 13: Z = 3,522 is still NQ 5, NQ 12 begins at need 6)
    for Z in (200, 1730, 3522, 4097, 10178):
        for cpt, cpz in NARROW_EDGES.items():
            add(f"heavy-nq{ladder_nq(HEAVY_K, need_of(Z))}-cpt{cpt}", Z, cpz, table="hot", kind="heavy")
    # sparse packs
    for cpt, cpz in WIDE_EDGES.items():
        add(f"sparse-two-cpt{cpt}", SPARSE_Z, cpz, table="sparse")
        add(f"sparse-one-cpt{cpt}", SPARSE_Z, cpz, table="sparse", fused=1, perm=True)
    for cpt, cpz in NARROW_EDGES.items():
        add(f"sparse-heavy-cpt{cpt}", SPARSE_Z, cpz, table="sparse", kind="heavy")
        for fused in (3, 6):
            add(f"sparse-form{fused}-cpt{cpt}", SPARSE_Z, cpz, table="sparse", fused=fused)
    # the secondary forms.  Placing first (3) and all hours in one launch (6): every (CPT, NQ <= 12), each cell being code of its own;
    # 8 runs the instantiations of 6 with another block order (a run-time argument): a cross, every NQ at CPT 1 and every CPT at NQ 1
    for fused in (3, 6, 8):
        for nq, (lo, hi) in sorted(bands.items()):
            if nq > 12:
                continue
            for cpt, cpz in NARROW_EDGES.items():
                if fused != 8 or cpt == 1 or nq == 1:
                    add(f"form{fused}-nq{nq}-cpt{cpt}", lo, cpz, fused=fused)
    # the batched sampler: two fleets, dense and sparse
    for cpt, cpz in WIDE_EDGES.items():
        add(f"batch-cpt{cpt}", 192, cpz, kind="batch")
        add(f"batch-sparse-cpt{cpt}", SPARSE_Z, cpz, table="sparse", kind="batch")
    add("batch-place1024", bands[40][0], 170, kind="batch")   # k_batch_place<1024, 4>: on the tables of the two-launch case there
    return tuple(out)


CASES = _cases()
OUT_OF_SCOPE = "Z = 32,768 (the upper edge of the NQ = 40 band) is not run: 17 GB of p_destin on the host at T = 2"


def case_steps(c):
    """[(what, options, predicted record)] of a case, in the order the test runs them; options: dict(last_hour, zone_order).
    Heavy cases: the records hold once the context has seen the heavy buckets (parts > 1)."""
    Z, T, n, sp = c.Z, c.T, c.Z * c.cpz, c.table == "sparse"
    if c.kind == "batch":
        return [("batch", dict(last_hour=lh), predict_batch(Z, n, T, sparse=sp, last_hour=lh)) for lh in (0, 1)]
    if c.kind == "heavy":
        return [("resample", {}, predict(Z, n, T, step="resample", parts=2, sparse=sp)),
                ("ivp", {}, predict(Z, n, T, step="ivp", parts=2, sparse=sp))]
    steps = [("ivp", dict(zone_order=0), predict(Z, n, T, step="ivp", fused=c.fused, sparse=sp, zone_order=0))]
    if c.fused == 0:
        for lh in (0, 1):
            steps.append(("resample", dict(last_hour=lh, zone_order=0), predict(Z, n, T, step="resample", sparse=sp, last_hour=lh, zone_order=0)))
    else:
        for zo in ((0, 1) if c.perm else (0,)):
            steps.append(("resample", dict(last_hour=1, zone_order=zo),
                          predict(Z, n, T, step="resample", fused=c.fused, sparse=sp, zone_order=zo, perm_valid=True)))
    return steps


def covered():
    return frozenset(w for c in CASES for (_, _, rec) in case_steps(c) for w in rec.values() if w)
