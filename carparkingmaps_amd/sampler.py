"""Sampler: thin object wrapper over the C ABI (include/cpm.h) with numpy arrays in the
reference's layout (Fortran order, 1-based zone ids).  One Sampler = one cpm_ctx = one GPU.
"""
import ctypes as C
import dataclasses
import os

import numpy as np

from . import _lib


def _f64(a, shape=None):
    a = np.asfortranarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclasses.dataclass
class ChargeParams:
    """The parameters of resample(charge=...) (include/cpm_charge.h): battery capacity in Wh, Wh a parked car takes per hour, every
    car's charge at hour 0, Wh per km driven; zone_power_wh: charger power per zone ((Z,) uint32, 0 = no charger) in place of
    power_wh; soc_in: initial charge per local car ((n,) uint32, clamped to the capacity) in place of initial_wh."""
    capacity_wh: int
    power_wh: int = 0
    initial_wh: int = 0
    wh_per_km: float = 0.0
    zone_power_wh: object = None
    soc_in: object = None


class Sampler:
    """Device-resident tables + car state for `number_zones` zones and T hours on one GPU."""

    def __init__(self, number_zones, T=24, device=0, stream=None):
        """stream: a HIP stream to enqueue on -- an integer handle or an object with `.cuda_stream` (torch.cuda.Stream), which is
        kept alive with the Sampler.  Given here, the context never creates a stream of its own: a process has few hardware
        queues (GPU_MAX_HW_QUEUES, 4 by default) and every HIP stream that is created takes a share of one, so two contexts
        meant to run side by side should each get their stream at construction (model_selection.grid_sweep over two lanes)."""
        self._L = _lib.load()
        self.Z, self.T, self.device = int(number_zones), int(T), int(device)
        h = C.c_void_p()
        _lib.check(self._L.cpm_create(C.byref(h), self.Z, self.T, self.device))
        self._h = h
        self._stream_obj = self._stream = None
        if stream is not None:
            self.set_stream(stream)
        self.C_total = self.cars_per_zone = self.car_begin = self.car_count = 0
        self.car_stride = 1

    # -- lifetime ----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.cpm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- options -----------------------------------------------------------
    def set_kernel(self, kernel):
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_KERNEL, int(kernel)))

    def set_fused(self, mode=1, lag=None):
        """The grouped path's fused hour: 5 on where it pays (the library's default), 1 on wherever it can run, 0 two launches per hour, 2 on with placing blocks that give up at once
        (tests), 3 the placing-first form (the previous hour's placing blocks in front of the hour's samplers), 4 = 3 with samplers
        that give up at once (tests); 6 all hours of a run in ONE launch (k_grouped_day: the placing blocks of an hour among the next
        hour's sampler workgroups, which draw for their stayers first), 8 = 6 with the placing blocks in front, 7 = 6 with blocks that
        give up at once (tests); lag: chunks of sampler workgroups in front of a chunk's placing blocks (mode 1)."""
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_FUSED, int(mode)))
        if lag is not None:
            _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_FUSED_LAG, int(lag)))

    def set_zone_order(self, on=True):
        """The one-launch hour deals its sampler workgroups the zones largest-first (a scheduling hint; the counts do not depend on
        it): 1 / True on, 0 / False off, 2 = the library's default: on for sparse row packs (datasets: -14 % at Melbourne's shape),
        off for dense ones (2-4 % slower at 4,096 zones)."""
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_ZONE_ORDER, int(on)))

    def set_sparse_upload(self, on=True):
        """set_p_dest gives an uploaded p_destin the sparse row packs build_p_dest gives a sparse datamatrix's tables, when the table
        qualifies (no row with more than 512 non-zero entries, the sparse pack at most 60 % of the dense one: include/cpm.h,
        CPM_OPT_SPARSE_UPLOAD); otherwise, and when off (the library's default), dense packs.  Read when a table is installed; the
        counts do not depend on it.  get_info(6) tells which form the installed table took."""
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_SPARSE_UPLOAD, 1 if on else 0))

    def set_last_hour(self, count_only=True):
        """Hour T of a grouped resample (sampled, never applied): True (the library's default) runs the count-only kernel wherever
        only the hour's counts are wanted, False the plain form of the full sampler.  The counts do not depend on it; get_info(11)
        tells what the most recent step ran."""
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_LAST_HOUR, 1 if count_only else 0))

    def set_narrow_pack(self, on=True):
        """The one-launch hour on dense row packs in zone order streams narrow packs (16 bracket-relative bits per destination instead
        of a 32-bit high word: include/cpm.h, CPM_OPT_NARROW_PACK) where the library's rule allows: True (the library's default), or
        False: wide packs everywhere.  The counts do not depend on it; narrow_pack() tells what the most recent step streamed."""
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_NARROW_PACK, 1 if on else 0))

    def narrow_pack(self):
        """1 when the applied hours of the most recent step streamed narrow row packs, from what was launched (CPM_INFO_NARROW_PACK)."""
        return self.get_info(_lib.CPM_INFO_NARROW_PACK)

    def narrow_ties(self):
        """Draws so far that a narrow pack's 16 bits could not decide and that read the wide words instead (CPM_INFO_NARROW_TIES).  A
        device word: the call BLOCKS until the context's stream has drained, so it must not be made while the stream is captured."""
        return self.get_info(_lib.CPM_INFO_NARROW_TIES)

    def get_info(self, what):
        """cpm_get_info (keys: _lib.CPM_INFO_*).  What the context would run next: 1 = kernel family AUTO resolves to now, 2 =
        bucket-region size in multiples of the mean bucket, 3 = workgroups per heavy zone, 4 = form of the hour (0 two launches, 1 one,
        3 placing first, 6 all hours in one launch), 5 = steps that bailed out of a one-launch form, 6 = words of a sparse row pack (0:
        dense tables; > 0 after build_p_dest on a sparse datamatrix or after set_p_dest under set_sparse_upload on a table that qualifies).  What its most recent step ran: 7 = the kernel family that produced its results (0 before any step), 8 = the
        form its grouped hours took (coded as 4; -1 when the family is not the grouped one), 9 = step attempts the library discarded
        and ran again so far, 11 = 1 when its hour T ran the count-only kernel (set_last_hour).  12 = the travel table the grouped path's
        travel kernel reads for the resident datamatrix (0 none built yet, 1 the dataset route's compact rows, 2 sparse rows, 3 the
        dense table it gathers from)."""
        v = C.c_int64(0)
        _lib.check(self._L.cpm_get_info(self._h, int(what), C.byref(v)))
        return int(v.value)

    def last_step(self):
        """The record of the most recent step: {kernel, form, repeats (cumulative), cap_mult, parts, bailouts (cumulative), batch_fleets
        (fleets of a batch step that the batched kernels produced; 0 after any other step), cells}.  `cells` names the instantiation
        each role of the step launched ({applied, heavy, last, place, batch}: _lib.CPM_INFO_CELL_*, words as include/cpm.h codes them,
        0 where the step had no such launch).
        Not a plain getter: an IVP that solve_ivp_async left in flight is committed first (the call waits for the stream and may
        repeat that IVP, which then shows in `repeats`), so it must not be called while the stream is being captured."""
        return dict(kernel=self.get_info(_lib.CPM_INFO_LAST_KERNEL), form=self.get_info(_lib.CPM_INFO_LAST_FORM),
                    repeats=self.get_info(_lib.CPM_INFO_STEPS_REPEATED), cap_mult=self.get_info(_lib.CPM_INFO_CAP_MULT),
                    parts=self.get_info(_lib.CPM_INFO_PARTS), bailouts=self.get_info(_lib.CPM_INFO_FUSED_BAILOUTS),
                    batch_fleets=self.get_info(_lib.CPM_INFO_LAST_BATCH_FLEETS),
                    cells=dict(applied=self.get_info(_lib.CPM_INFO_CELL_APPLIED), heavy=self.get_info(_lib.CPM_INFO_CELL_HEAVY),
                               last=self.get_info(_lib.CPM_INFO_CELL_LAST), place=self.get_info(_lib.CPM_INFO_CELL_PLACE),
                               batch=self.get_info(_lib.CPM_INFO_CELL_BATCH)))

    def set_profile(self, on=True, stride=1, kernel=0):
        """hipEvents around every `stride`-th hourly launch of `kernel` (0 sampler, 1 place, 2 travel; 3: the two kernels of a
        sparse upload, per set_p_dest); on=False: off."""
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_PROFILE_KERNEL, int(kernel)))
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_PROFILE, int(stride) if on else 0))

    def set_stream(self, hip_stream):
        """hip_stream: integer handle (e.g. torch.cuda.current_stream().cuda_stream), an object with `.cuda_stream`, or None."""
        handle = getattr(hip_stream, "cuda_stream", hip_stream)
        _lib.check(self._L.cpm_set_stream(self._h, C.c_void_p(handle) if handle else None))
        self._stream_obj, self._stream = (hip_stream if handle else None), (handle or None)

    def sync(self):
        _lib.check(self._L.cpm_sync(self._h))

    # -- tables ------------------------------------------------------------
    def set_p_drive(self, p_drive):
        a = _f64(p_drive, (self.Z, self.T))
        _lib.check(self._L.cpm_set_p_drive(self._h, _vp(a)))

    def set_p_dest(self, p_dest):
        a = _f64(p_dest, (self.Z, self.Z, self.T))
        _lib.check(self._L.cpm_set_p_dest(self._h, _vp(a)))

    def set_datamatrix(self, datamatrix, distance_matrix_km=None):
        """distance_matrix_km None: the distance matrix already resident (set_distance*) is kept."""
        a = _f64(datamatrix, (self.Z, self.Z, self.T, 2))
        d = None if distance_matrix_km is None else _f64(distance_matrix_km, (self.Z, self.Z))
        _lib.check(self._L.cpm_set_datamatrix(self._h, _vp(a), _vp(d)))

    def createdatamatrix_rows(self, rawdata):
        """rawdata: (n, 5) = the reference's rawdata[:,1:5]; builds the dense datamatrix in HBM."""
        a = np.asfortranarray(rawdata, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError(f"expected (n, 5) rows, got {a.shape}")
        _lib.check(self._L.cpm_createdatamatrix_rows(self._h, int(a.shape[0]), _vp(a)))

    def createdatamatrix_csv(self, path):
        """Uber Movement CSV -> dense datamatrix in HBM (native parser); returns the number of data rows."""
        n = C.c_int64(0)
        _lib.check(self._L.cpm_createdatamatrix_csv(self._h, os.fsencode(path), C.byref(n)))
        return int(n.value)

    def get_datamatrix(self):
        out = np.zeros((self.Z, self.Z, self.T, 2), dtype=np.float64, order="F")
        _lib.check(self._L.cpm_get_datamatrix(self._h, _vp(out)))
        return out

    def set_distance_from_centroids(self, centroid_lat, centroid_long):
        la = np.ascontiguousarray(centroid_lat, dtype=np.float64).reshape(-1)
        lo = np.ascontiguousarray(centroid_long, dtype=np.float64).reshape(-1)
        if la.shape != (self.Z,) or lo.shape != (self.Z,):
            raise ValueError(f"expected {self.Z} centroids")
        _lib.check(self._L.cpm_set_distance_from_centroids(self._h, _vp(la), _vp(lo)))

    def set_distance(self, distance_matrix_km):
        d = _f64(distance_matrix_km, (self.Z, self.Z))
        _lib.check(self._L.cpm_set_distance(self._h, _vp(d)))

    def get_distance(self):
        out = np.zeros((self.Z, self.Z), dtype=np.float64, order="F")
        _lib.check(self._L.cpm_get_distance(self._h, _vp(out)))
        return out

    def build_p_drive(self, p_min, p_max, e_drive, want=True):
        out = np.zeros((self.Z, self.T), dtype=np.float64, order="F") if want else None
        _lib.check(self._L.cpm_build_p_drive(self._h, float(p_min), float(p_max), float(e_drive), _vp(out)))
        return out

    def build_p_dest(self, e_dest, want=True):
        out = np.zeros((self.Z, self.Z, self.T), dtype=np.float64, order="F") if want else None
        is_int = int(isinstance(e_dest, (int, np.integer)) and not isinstance(e_dest, bool))
        _lib.check(self._L.cpm_build_p_dest(self._h, float(e_dest), is_int, _vp(out)))
        return out

    def synth_tables(self, table_seed, skew_q=0):
        """Procedural bench tables; skew_q > 0: destination popularity 1 / (skew_q + rank), see include/cpm.h."""
        _lib.check(self._L.cpm_synth_tables_skewed(self._h, int(table_seed), int(skew_q)))

    def synth_datamatrix(self, table_seed, density=0.0868):
        """Melbourne-shaped synthetic datamatrix + distance matrix, generated on the device."""
        _lib.check(self._L.cpm_synth_datamatrix(self._h, int(table_seed), float(density)))

    def refresh_tables(self, with_f64_cdf=False):
        """Re-derive the row tables from the resident p_destin -- or from the compact rows of the dataset they were built from -- (the one
        pass the installing calls end in); for measurement."""
        _lib.check(self._L.cpm_refresh_tables(self._h, 1 if with_f64_cdf else 0))

    def get_p_drive(self):
        out = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        _lib.check(self._L.cpm_get_p_drive(self._h, _vp(out)))
        return out

    def get_cdf_row(self, origin, hour):
        out = np.zeros(self.Z, dtype=np.float64)
        _lib.check(self._L.cpm_get_cdf_row(self._h, int(origin), int(hour), _vp(out)))
        return out

    # -- cars --------------------------------------------------------------
    def init_states(self, C_total, cars_per_zone, car_begin=0, car_count=None, car_stride=1):
        """This context simulates the global cars car_begin + k * car_stride, k < car_count (stride 1: a contiguous range)."""
        car_stride = int(car_stride)
        if car_count is None:
            car_count = max(0, -(-(int(C_total) - int(car_begin)) // car_stride))
        car_count = int(car_count)
        _lib.check(self._L.cpm_init_states_strided(self._h, int(C_total), int(cars_per_zone), int(car_begin), car_stride, car_count))
        self.C_total, self.cars_per_zone = int(C_total), int(cars_per_zone)
        self.car_begin, self.car_count, self.car_stride = int(car_begin), car_count, car_stride

    def set_state(self, zones):
        z = np.ascontiguousarray(zones, dtype=np.int64)
        if z.shape != (self.car_count,):
            raise ValueError(f"expected {self.car_count} zones, got {z.shape}")
        _lib.check(self._L.cpm_set_state(self._h, _vp(z)))

    def get_state(self):
        out = np.zeros(self.car_count, dtype=np.int64)
        _lib.check(self._L.cpm_get_state(self._h, _vp(out)))
        return out

    def solve_ivp(self, seed, want=True):
        out = np.zeros(self.car_count, dtype=np.int64) if want else None
        _lib.check(self._L.cpm_solve_ivp(self._h, int(seed), _vp(out)))
        return out

    def solve_ivp_async(self, seed):
        _lib.check(self._L.cpm_solve_ivp_async(self._h, int(seed)))

    def resample(self, seed, travel=False, want_state=False, want_trans=False, flows=False, stays=False, paths=False, charge=None):
        """Returns dict(parking, driving: (Z,T) int64 F-order; sum_tt_q16: int; state, trans or None).
        flows=True (include/cpm_flows.h): the dict gains `flows`, the OD trip counts of every hour: (T, Z, Z) int32, C order,
        flows[t, o, d] = cars that drove from zone o + 1 to zone d + 1 in hour t + 1 (trips inside a zone on the diagonal), from the
        kernel family that produced the counts.  Not together with want_state / want_trans, which force the per-car kernels.
        flows="csr" (include/cpm_flows_csr.h): the dict gains `flows_csr` instead, the same counts without the zeros:
        dict(row_ptr (T*Z + 1,) int64, dest (nnz,) int32, count (nnz,) int32, shape=(T, Z, Z)), row t*Z + o, destinations 0-based and
        ascending within a row (flows_csr_to_dense, flows_csr_hour).
        stays=True (include/cpm_stays.h): the dict gains `stays`, (T, Z, T) int32, C order, stays[t, z, L] = cars that drove out of (or
        within) zone z + 1 in hour t (0-based) after L whole parked hours there (L == t: parked since the day began), and `parked`,
        (Z, T) int32, parked[z, a] = cars parked in zone z + 1 since hour a that did not drive in the last hour (stay_length_histogram).
        Not together with flows, want_state or want_trans.
        paths=True (include/cpm_paths.h): the dict gains `paths`, (T, n) uint32, C order, n the context's car count:
        paths[t, i] = (destination of car i in hour t, 0-based; its own zone when it did not drive) | 0x80000000 when it drove, from
        the kernel family that produced the counts (paths_to_matrices, paths_flows).  Not together with flows, stays, want_state or
        want_trans.
        charge=ChargeParams(...) or a dict of its fields (include/cpm_charge.h): the dict gains `charge`, (Z, T) int64, C order,
        charge[z, t] = Wh the chargers of zone z + 1 delivered in hour t; `used`, (Z, T) int64, Wh taken from batteries by the trips
        that start in zone z + 1 in hour t; `short`, (Z, T) int32, those trips the battery did not cover; and `soc`, (n,) uint32, every
        car's charge when the day ends.  Needs a resident distance matrix.  Not together with flows, stays, paths, want_state or
        want_trans."""
        parking = np.zeros((self.Z, self.T), dtype=np.int64, order="F")
        driving = np.zeros((self.Z, self.T), dtype=np.int64, order="F")
        if charge is not None:
            if flows or stays or paths or want_state or want_trans:
                raise ValueError("charge cannot be combined with flows, stays, paths, want_state or want_trans")
            params, keep = self._charge_params(charge)
            out, used, short, soc = self.charge_empty(), self.used_empty(), self.short_empty(), self.soc_empty()
            tt = C.c_int64(0)
            _lib.check(self._L.cpm_resample_charge(self._h, int(seed), _lib.CPM_FLAG_TRAVEL if travel else 0, C.byref(params), _vp(parking),
                                                   _vp(driving), C.cast(C.byref(tt), C.c_void_p), _vp(out), _vp(used), _vp(short), _vp(soc)))
            del keep
            return dict(parking=parking, driving=driving, sum_tt_q16=int(tt.value), state=None, trans=None, charge=out, used=used,
                        short=short, soc=soc)
        if paths:
            if flows or stays or want_state or want_trans:
                raise ValueError("paths=True cannot be combined with flows, stays, want_state or want_trans")
            out = self.paths_empty()
            tt = C.c_int64(0)
            _lib.check(self._L.cpm_resample_paths(self._h, int(seed), _lib.CPM_FLAG_TRAVEL if travel else 0, _vp(parking), _vp(driving),
                                                  C.cast(C.byref(tt), C.c_void_p), _vp(out)))
            return dict(parking=parking, driving=driving, sum_tt_q16=int(tt.value), state=None, trans=None, paths=out)
        if stays:
            if flows or want_state or want_trans:
                raise ValueError("stays=True cannot be combined with flows, want_state or want_trans")
            out, parked = self.stays_empty(), self.parked_empty()
            tt = C.c_int64(0)
            _lib.check(self._L.cpm_resample_stays(self._h, int(seed), _lib.CPM_FLAG_TRAVEL if travel else 0, _vp(parking), _vp(driving),
                                                  C.cast(C.byref(tt), C.c_void_p), _vp(out), _vp(parked)))
            return dict(parking=parking, driving=driving, sum_tt_q16=int(tt.value), state=None, trans=None, stays=out, parked=parked)
        if isinstance(flows, str):
            if flows != "csr":
                raise ValueError(f"flows={flows!r}: expected False, True or \"csr\"")
            if want_state or want_trans:
                raise ValueError("flows=\"csr\" cannot be combined with want_state / want_trans")
            row_ptr = np.empty(self.T * self.Z + 1, dtype=np.int64)
            tt, nnz = C.c_int64(0), C.c_int64(0)
            _lib.check(self._L.cpm_resample_flows_csr(self._h, int(seed), _lib.CPM_FLAG_TRAVEL if travel else 0, _vp(parking), _vp(driving),
                                                      C.cast(C.byref(tt), C.c_void_p), _vp(row_ptr), C.byref(nnz)))
            dest = np.empty(nnz.value, dtype=np.int32)    # (sized by the first call, fetched by the second: no guess, no retry)
            count = np.empty(nnz.value, dtype=np.int32)
            _lib.check(self._L.cpm_get_flows_csr(self._h, _vp(dest), _vp(count), nnz.value))
            return dict(parking=parking, driving=driving, sum_tt_q16=int(tt.value), state=None, trans=None,
                        flows_csr=dict(row_ptr=row_ptr, dest=dest, count=count, shape=(self.T, self.Z, self.Z)))
        if flows:
            if want_state or want_trans:
                raise ValueError("flows=True cannot be combined with want_state / want_trans")
            out = self.flows_empty()
            tt = C.c_int64(0)
            _lib.check(self._L.cpm_resample_flows(self._h, int(seed), _lib.CPM_FLAG_TRAVEL if travel else 0, _vp(parking), _vp(driving),
                                                  C.cast(C.byref(tt), C.c_void_p), _vp(out)))
            return dict(parking=parking, driving=driving, sum_tt_q16=int(tt.value), state=None, trans=None, flows=out)
        state = np.zeros((self.car_count, self.T), dtype=np.int64, order="F") if want_state else None
        trans = np.zeros((self.car_count, self.T, 4), dtype=np.float64, order="F") if want_trans else None
        tt = C.c_int64(0)
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample(self._h, int(seed), flags, _vp(parking), _vp(driving),
                                        C.cast(C.byref(tt), C.c_void_p), _vp(state), _vp(trans)))
        return dict(parking=parking, driving=driving, sum_tt_q16=int(tt.value), state=state, trans=trans)

    def resample_dev(self, seed, d_counts_ptr, travel=False):
        """Enqueue on the context's stream; d_counts_ptr = device address of int64[2*T*Z+2]
        (parking | driving | sum_tt_q16 | status; status != 0 -> repeat with another kernel)."""
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample_dev(self._h, int(seed), flags, C.c_void_p(int(d_counts_ptr))))

    def counts_words(self):
        return 2 * self.T * self.Z + 2

    # -- OD trip counts (include/cpm_flows.h) --
    def flows_words(self):
        """int32 words of the flows tensor: T * Z * Z."""
        return self.T * self.Z * self.Z

    def flows_empty(self):
        """The host array resample(flows=True) fills: (T, Z, Z) int32, C order (the library writes every word)."""
        return np.empty((self.T, self.Z, self.Z), dtype=np.int32, order="C")

    def resample_flows_dev(self, seed, d_counts_ptr, d_flows_ptr, travel=False):
        """Enqueue on the context's stream; d_counts_ptr as for resample_dev, d_flows_ptr = device address of int32[T*Z*Z]
        (flows[t][o][d]).  A non-zero status word in the count tensor invalidates the flows as well: repeat the step."""
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample_flows_dev(self._h, int(seed), flags, C.c_void_p(int(d_counts_ptr)), C.c_void_p(int(d_flows_ptr))))

    def resample_flows_csr_dev(self, seed, d_counts_ptr, d_row_ptr, d_dest, d_count, cap, travel=False):
        """Enqueue on the context's stream (include/cpm_flows_csr.h); d_counts_ptr as for resample_dev, d_row_ptr = device address of
        int64[T*Z + 1], d_dest / d_count = device addresses of int32[cap] (0 with cap = 0: size only).  row_ptr is always complete:
        row_ptr[T*Z] is the size the step needs; entries below cap are valid, nothing is stored behind it.  A non-zero status word in
        the count tensor invalidates all three arrays: repeat the step."""
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample_flows_csr_dev(self._h, int(seed), flags, C.c_void_p(int(d_counts_ptr)), C.c_void_p(int(d_row_ptr)),
                                                      C.c_void_p(int(d_dest)) if d_dest else None, C.c_void_p(int(d_count)) if d_count else None,
                                                      int(cap)))

    def set_flows_kept(self, on=True):
        """How the grouped family computes the flows: one launch over the kept runs of all hours (True) or one behind every hour
        (False, the library's default; measured in DESIGN.md 8).  The flows do not depend on it."""
        _lib.check(self._L.cpm_set_option(self._h, _lib.CPM_OPT_FLOWS_KEPT, 1 if on else 0))

    # -- parking stays (include/cpm_stays.h) --
    def stays_empty(self):
        """The host array resample(stays=True) fills with the completed stays: (T, Z, T) int32, C order (the library writes every word)."""
        return np.empty((self.T, self.Z, self.T), dtype=np.int32, order="C")

    def parked_empty(self):
        """The host array resample(stays=True) fills with the stays still open at the end of the day: (Z, T) int32, C order."""
        return np.empty((self.Z, self.T), dtype=np.int32, order="C")

    def resample_stays_dev(self, seed, d_counts_ptr, d_stays_ptr, d_parked_ptr, travel=False):
        """Enqueue on the context's stream; d_counts_ptr as for resample_dev, d_stays_ptr = device address of int32[T*Z*T]
        (stays[t][z][L]), d_parked_ptr = device address of int32[Z*T] (parked[z][a]).  A non-zero status word in the count tensor
        invalidates both arrays: repeat the step."""
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample_stays_dev(self._h, int(seed), flags, C.c_void_p(int(d_counts_ptr)), C.c_void_p(int(d_stays_ptr)),
                                                  C.c_void_p(int(d_parked_ptr))))

    # -- charge (include/cpm_charge.h) --
    def _charge_params(self, charge):
        """(the C struct of a ChargeParams or a dict of its fields with host arrays, the arrays it points to)"""
        p = charge if isinstance(charge, ChargeParams) else ChargeParams(**charge)
        zp = None if p.zone_power_wh is None else np.ascontiguousarray(p.zone_power_wh, dtype=np.uint32)
        si = None if p.soc_in is None else np.ascontiguousarray(p.soc_in, dtype=np.uint32)
        if zp is not None and zp.shape != (self.Z,):
            raise ValueError(f"zone_power_wh: expected ({self.Z},), got {zp.shape}")
        if si is not None and si.shape != (self.car_count,):
            raise ValueError(f"soc_in: expected ({self.car_count},), got {si.shape}")
        c = _lib.ChargeParamsC(int(p.capacity_wh), int(p.power_wh), int(p.initial_wh), float(p.wh_per_km),
                               None if zp is None else zp.ctypes.data, None if si is None else si.ctypes.data)
        return c, (zp, si)

    def charge_empty(self):
        """The host array resample(charge=...) fills with the charging load: (Z, T) int64, C order (the library writes every word)."""
        return np.empty((self.Z, self.T), dtype=np.int64, order="C")

    def used_empty(self):
        """The host array resample(charge=...) fills with the energy the trips took: (Z, T) int64, C order."""
        return np.empty((self.Z, self.T), dtype=np.int64, order="C")

    def short_empty(self):
        """The host array resample(charge=...) fills with the trips the battery did not cover: (Z, T) int32, C order."""
        return np.empty((self.Z, self.T), dtype=np.int32, order="C")

    def soc_empty(self):
        """The host array resample(charge=...) fills with every car's charge at the end of the day: (n,) uint32."""
        return np.empty((self.car_count,), dtype=np.uint32)

    def resample_charge_dev(self, seed, d_counts_ptr, d_charge_ptr, d_used_ptr, d_short_ptr, d_soc_ptr, capacity_wh, power_wh=0, initial_wh=0,
                            wh_per_km=0.0, d_zone_power_ptr=0, d_soc_in_ptr=0, travel=False):
        """Enqueue on the context's stream; d_counts_ptr as for resample_dev, d_charge_ptr / d_used_ptr = device addresses of
        int64[Z*T], d_short_ptr of int32[Z*T], d_soc_ptr of uint32[n] or 0; d_zone_power_ptr / d_soc_in_ptr = device addresses of
        uint32[Z] / uint32[n] or 0, which must stay valid until the step has run.  A non-zero status word in the count tensor
        invalidates all four arrays: repeat the step."""
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        p = _lib.ChargeParamsC(int(capacity_wh), int(power_wh), int(initial_wh), float(wh_per_km), int(d_zone_power_ptr) or None,
                               int(d_soc_in_ptr) or None)
        _lib.check(self._L.cpm_resample_charge_dev(self._h, int(seed), flags, C.byref(p), C.c_void_p(int(d_counts_ptr)) if d_counts_ptr else None,
                                                   C.c_void_p(int(d_charge_ptr)) if d_charge_ptr else None,
                                                   C.c_void_p(int(d_used_ptr)) if d_used_ptr else None,
                                                   C.c_void_p(int(d_short_ptr)) if d_short_ptr else None,
                                                   C.c_void_p(int(d_soc_ptr)) if d_soc_ptr else None))

    # -- per-car day records (include/cpm_paths.h) --
    def paths_words(self):
        """uint32 words of the record: T * n, n the context's car count."""
        return self.T * self.car_count

    def paths_empty(self):
        """The host array resample(paths=True) fills: (T, n) uint32, C order (the library writes every word)."""
        return np.empty((self.T, self.car_count), dtype=np.uint32, order="C")

    def resample_paths_dev(self, seed, d_counts_ptr, d_paths_ptr, travel=False):
        """Enqueue on the context's stream; d_counts_ptr as for resample_dev, d_paths_ptr = device address of uint32[T*n]
        (paths[t][i]).  A non-zero status word in the count tensor invalidates the record: repeat the step."""
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample_paths_dev(self._h, int(seed), flags, C.c_void_p(int(d_counts_ptr)) if d_counts_ptr else None,
                                                  C.c_void_p(int(d_paths_ptr)) if d_paths_ptr else None))

    def paths_expand_dev(self, seed, d_paths_ptr, d_state_ptr, d_trans_ptr, travel=False):
        """Enqueue on the context's stream: the reference's matrices from a record, on the device.  d_state_ptr = device address of
        int64[T*n] (state_matrix, C x T column-major, 1-based) or 0, d_trans_ptr = device address of float64[4*T*n]
        (transition_matrix, C x T x 4 column-major) or 0.  The context's state and the seed must be those of the step that produced
        the record; travel=True re-derives the travel-time and distance columns, which are zero otherwise."""
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_paths_expand_dev(self._h, int(seed), flags, C.c_void_p(int(d_paths_ptr)) if d_paths_ptr else None,
                                                C.c_void_p(int(d_state_ptr)) if d_state_ptr else None,
                                                C.c_void_p(int(d_trans_ptr)) if d_trans_ptr else None))

    # -- batches (include/cpm_batch.h): B fleets, each with its own p_drive and seed, from this context's state and p_destin --
    def set_p_drive_batch(self, p_drives):
        """p_drives: (Z, T, B), B <= 64 (Julia p_drives[:,:,b]); replaces the batch tables.  The context's own p_drive is untouched."""
        a = np.asfortranarray(p_drives, dtype=np.float64)
        if a.ndim != 3 or a.shape[:2] != (self.Z, self.T):
            raise ValueError(f"expected shape ({self.Z}, {self.T}, B), got {a.shape}")
        _lib.check(self._L.cpm_set_p_drive_batch(self._h, int(a.shape[2]), _vp(a)))

    def build_p_drive_batch(self, p_min, p_max, e_drive, want=False):
        """createpdrive once per fleet: fleet b = (p_min[b], p_max[b], e_drive[b]).  want: also return the (Z, T, B) tables."""
        cols = [np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (p_min, p_max, e_drive)]
        B = cols[0].shape[0]
        if any(c.shape != (B,) for c in cols):
            raise ValueError("p_min, p_max and e_drive must be sequences of one length")
        _lib.check(self._L.cpm_build_p_drive_batch(self._h, int(B), *(_vp(c) for c in cols)))
        return self.get_p_drive_batch() if want else None

    def get_p_drive_batch(self):
        out = np.zeros((self.Z, self.T, self.get_info(_lib.CPM_INFO_BATCH)), dtype=np.float64, order="F")
        _lib.check(self._L.cpm_get_p_drive_batch(self._h, _vp(out)))
        return out

    def _batch_seeds(self, seeds):
        B = self.get_info(_lib.CPM_INFO_BATCH)
        sd = np.asarray(seeds, dtype=np.uint64).reshape(-1)
        if sd.shape[0] == 1:
            sd = np.full(B, sd[0], dtype=np.uint64)
        if sd.shape[0] != B:
            raise ValueError(f"{sd.shape[0]} seeds for {B} fleets")
        return np.ascontiguousarray(sd), B

    def resample_batch(self, seeds, travel=False):
        """Every fleet of the installed batch tables, blocking.  seeds: one for all fleets (common random numbers) or B.  Returns
        dict(parking, driving: (Z, T, B) int64 F-order; sum_tt_q16: (B,) int64) -- fleet b bit for bit resample(seeds[b]) with
        p_drive[:, :, b] installed."""
        sd, B = self._batch_seeds(seeds)
        parking = np.zeros((self.Z, self.T, B), dtype=np.int64, order="F")
        driving = np.zeros((self.Z, self.T, B), dtype=np.int64, order="F")
        tt = np.zeros(B, dtype=np.int64)
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample_batch(self._h, _vp(sd), flags, _vp(parking), _vp(driving), _vp(tt)))
        return dict(parking=parking, driving=driving, sum_tt_q16=tt)

    def resample_batch_dev(self, seeds, d_counts_ptr, travel=False):
        """Enqueue on the context's stream; d_counts_ptr = device address of int64[B][2*T*Z+2], each fleet laid out like
        resample_dev's tensor with its own status word (!= 0: that fleet's counts are invalid, repeat it)."""
        sd, _ = self._batch_seeds(seeds)
        flags = _lib.CPM_FLAG_TRAVEL if travel else 0
        _lib.check(self._L.cpm_resample_batch_dev(self._h, _vp(sd), flags, C.c_void_p(int(d_counts_ptr))))

    def batch_counts_words(self):
        """int64 words of resample_batch_dev's tensor: B x counts_words()."""
        return self.get_info(_lib.CPM_INFO_BATCH) * self.counts_words()

    # -- the sweep's objectives on the device (include/cpm_objectives.h) --
    def set_measured(self, parking_density_measured):
        """The measured parking densities, (Z, T), resident until replaced; None: forget them.  NaN or infinite entries raise."""
        if parking_density_measured is None:
            _lib.check(self._L.cpm_set_measured(self._h, None))
            return
        a = _f64(parking_density_measured, (self.Z, self.T))
        _lib.check(self._L.cpm_set_measured(self._h, _vp(a)))

    def objective_words(self):
        """int64 words of one fleet's record: 4 + 2*T (status, sum_tt_q16, n_valid, bits of the f64 parking_error, driving_sum[T],
        parking_sum[T])."""
        return 4 + 2 * self.T

    def objectives_dev(self, d_counts_ptr, B, n_cars, d_obj_ptr, d_zone_err_ptr=0):
        """Enqueue on the context's stream: the records of B count tensors (d_counts_ptr = device address of int64[B][2*T*Z+2], as
        resample_dev / resample_batch_dev fill it) into d_obj_ptr = device address of int64[B][objective_words()]; d_zone_err_ptr =
        device address of float64[B][Z] (the zones' errors, -1.0 where a zone is not valid) or 0.  n_cars: the cars whose counts a
        tensor holds (the fleet's behind an all-reduce).  No synchronisation."""
        _lib.check(self._L.cpm_objectives_dev(self._h, C.c_void_p(int(d_counts_ptr)) if d_counts_ptr else None, int(B), int(n_cars),
                                              C.c_void_p(int(d_obj_ptr)) if d_obj_ptr else None,
                                              C.c_void_p(int(d_zone_err_ptr)) if d_zone_err_ptr else None))

    # -- expected densities by Markov propagation (include/cpm_expected.h): no cars, no random numbers --
    def _pi0(self, pi0):
        return None if pi0 is None else np.ascontiguousarray(_f64(pi0, (self.Z,)))

    def expected(self, pi0=None, ivp=False, want_next=False, sparse=False):
        """The mean of the sampler's chain from the installed tables, blocking: (parking_density, driving_density), each (Z, T)
        float64 F-order; parking_density[:, t] = pi_t, driving_density = pi_t * p_drive as the Bernoulli maps it.  C * these are
        the expected counts of resample().  pi0: (Z,) or None (uniform 1/Z); ivp: start the day from pi0 carried through hours
        0 .. T-2 (the expected solve_ivp).  want_next: also return pi after the day's last operator.  sparse: straight from the
        compact rows of sparse tables (include/cpm_expected_sparse.h): the same bits, the dense p_destin array neither read nor built."""
        a = self._pi0(pi0)
        parking = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        driving = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        nxt = np.zeros(self.Z, dtype=np.float64) if want_next else None
        call = self._L.cpm_expected_sparse if sparse else self._L.cpm_expected
        _lib.check(call(self._h, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(parking), _vp(driving), _vp(nxt)))
        return (parking, driving, nxt) if want_next else (parking, driving)

    def expected_batch(self, pi0=None, ivp=False, sparse=False):
        """The same for every fleet of the installed batch tables: (parking_density, driving_density), each (Z, T, B); fleet b bit
        for bit expected() with p_drive[:, :, b] installed.  sparse: as in expected()."""
        a = self._pi0(pi0)
        B = self.get_info(_lib.CPM_INFO_BATCH)
        parking = np.zeros((self.Z, self.T, B), dtype=np.float64, order="F")
        driving = np.zeros((self.Z, self.T, B), dtype=np.float64, order="F")
        call = self._L.cpm_expected_sparse_batch if sparse else self._L.cpm_expected_batch
        _lib.check(call(self._h, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(parking), _vp(driving)))
        return parking, driving

    def expected_words(self):
        """float64 words of one fleet's expected_dev tensor: 2*T*Z (parking[T][Z], then driving[T][Z])."""
        return 2 * self.T * self.Z

    def expected_dev(self, d_out_ptr, d_pi0_ptr=0, ivp=False, d_pi_next_ptr=0, sparse=False):
        """Enqueue on the context's stream: d_out_ptr = device address of float64[expected_words()]; d_pi0_ptr = device address of
        float64[Z] or 0 (uniform); d_pi_next_ptr = device address of float64[Z] or 0.  (The first call after the p_destin tables
        changed builds its per-table arrays and synchronises once.)  sparse: cpm_expected_sparse_dev, as in expected()."""
        call = self._L.cpm_expected_sparse_dev if sparse else self._L.cpm_expected_dev
        _lib.check(call(self._h, C.c_void_p(int(d_pi0_ptr)) if d_pi0_ptr else None, _lib.CPM_EXPECT_IVP if ivp else 0,
                        C.c_void_p(int(d_out_ptr)) if d_out_ptr else None, C.c_void_p(int(d_pi_next_ptr)) if d_pi_next_ptr else None))

    # -- exact variances of the counts from the day's transition matrix (include/cpm_expected_var.h) --
    def expected_var(self, start=None, ivp=False):
        """Mean and exact variance of resample()'s counts over the seed, given the cars' start zones, blocking: a dict of four
        (Z, T) float64 F-order arrays, mean_parking, mean_driving, var_parking, var_driving.  start: (Z,) cars that start in each
        zone, or None (1 per zone); the outputs are linear in it.  After init_states(C, cars_per_zone) start is
        np.full(Z, cars_per_zone); for any other state it is np.bincount(get_state() - 1, minlength=Z) (get_state() is 1-based).
        ivp: the variances of solve_ivp() followed by resample(), given the placement in front of the IVP.  The standard error of a
        count is sqrt(var); model_selection.count_zscores() applies it."""
        a = None if start is None else np.ascontiguousarray(_f64(start, (self.Z,)))
        out = {k: np.zeros((self.Z, self.T), dtype=np.float64, order="F") for k in ("mean_parking", "mean_driving", "var_parking", "var_driving")}
        _lib.check(self._L.cpm_expected_var(self._h, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(out["mean_parking"]), _vp(out["mean_driving"]),
                                            _vp(out["var_parking"]), _vp(out["var_driving"])))
        return out

    def expected_var_words(self):
        """float64 words of the expected_var_dev tensor: 4*T*Z (mean_parking[T][Z], mean_driving, var_parking, var_driving)."""
        return 4 * self.T * self.Z

    def expected_var_dev(self, d_out_ptr, d_start_ptr=0, ivp=False):
        """Enqueue on the context's stream: d_out_ptr = device address of float64[expected_var_words()]; d_start_ptr = device address
        of float64[Z] (the cars that start in each zone: cars_per_zone of init_states, or np.bincount of get_state()) or 0 (1 per
        zone).  (The first call after the p_destin tables changed builds its per-table arrays and synchronises once.)"""
        _lib.check(self._L.cpm_expected_var_dev(self._h, C.c_void_p(int(d_start_ptr)) if d_start_ptr else None, _lib.CPM_EXPECT_IVP if ivp else 0,
                                                C.c_void_p(int(d_out_ptr)) if d_out_ptr else None))

    # -- the exact seed variance of linear functionals of the counts (include/cpm_expected_linear_var.h) --
    def expected_linear_var(self, a_parking, b_driving, start=None, ivp=False, per_zone=False, sparse=False):
        """Exact mean and variance over the seed of L = sum(a_parking * parking) + sum(b_driving * driving) of resample()'s (Z, T)
        count arrays, given the cars' start zones, blocking: one backward pass over the p_destin tables, with every covariance between
        zones and between hours in it.  a_parking / b_driving: (Z, T), or (Z, T, K) for K functionals (at most CPM_MAX_BATCH) in one
        call; functional k carries the bits of a call on it alone.  start, ivp: as in expected_var().  Returns dict(mean, var): floats
        for (Z, T) inputs, (K,) arrays otherwise; per_zone: also zone_mean, zone_var ((Z,) or (Z, K)): the mean and the variance one
        car that starts in each zone contributes -- mean = start @ zone_mean, var = start @ zone_var.  sparse: from the compact rows of
        sparse tables (include/cpm_expected_sparse_var.h): the same bits, the dense p_destin array neither read nor built."""
        a, b = np.asarray(a_parking, dtype=np.float64), np.asarray(b_driving, dtype=np.float64)
        single = a.ndim == 2
        if a.shape != b.shape or a.ndim not in (2, 3) or a.shape[:2] != (self.Z, self.T) or (a.ndim == 3 and a.shape[2] < 1):
            raise ValueError(f"expected_linear_var: coefficients {a.shape} and {b.shape}, expected two of ({self.Z}, {self.T}) or ({self.Z}, {self.T}, K)")
        K = 1 if single else a.shape[2]
        a, b = np.asfortranarray(a.reshape(self.Z, self.T, K, order="F")), np.asfortranarray(b.reshape(self.Z, self.T, K, order="F"))
        w = None if start is None else np.ascontiguousarray(_f64(start, (self.Z,)))
        mean, var = np.zeros(K), np.zeros(K)
        zm = np.zeros((self.Z, K), order="F") if per_zone else None
        zv = np.zeros((self.Z, K), order="F") if per_zone else None
        call = self._L.cpm_expected_sparse_linear_var if sparse else self._L.cpm_expected_linear_var
        _lib.check(call(self._h, _vp(w), _lib.CPM_EXPECT_IVP if ivp else 0, K, _vp(a), _vp(b), _vp(mean), _vp(var), _vp(zm), _vp(zv)))
        out = {"mean": float(mean[0]), "var": float(var[0])} if single else {"mean": mean, "var": var}
        if per_zone:
            out["zone_mean"], out["zone_var"] = (zm[:, 0], zv[:, 0]) if single else (zm, zv)
        return out

    def expected_linear_var_dev(self, K, d_coeff_ptr, d_out_ptr, d_start_ptr=0, ivp=False, d_zone_ptr=0, sparse=False):
        """Enqueue on the context's stream: d_coeff_ptr = device address of float64[K][2][T][Z] (A_k then B_k, the layout of
        expected_grad_dev's cotangent); d_out_ptr = device address of float64[K][2] (mean, variance); d_start_ptr = device address of
        float64[Z] or 0 (1 per zone); d_zone_ptr = device address of float64[K][2][Z] (per start zone) or 0.  (The first call after the
        p_destin tables changed builds its per-table arrays and synchronises once.)  sparse: as in expected_linear_var(); the
        coefficients must be finite (this call does not check them)."""
        p = lambda v: C.c_void_p(int(v)) if v else None
        call = self._L.cpm_expected_sparse_linear_var_dev if sparse else self._L.cpm_expected_linear_var_dev
        _lib.check(call(self._h, p(d_start_ptr), _lib.CPM_EXPECT_IVP if ivp else 0, int(K), p(d_coeff_ptr), p(d_out_ptr), p(d_zone_ptr)))

    # -- the exact seed variance of travel seconds, km and count functionals together (include/cpm_expected_travel_var.h) --
    def expected_trip_var(self, sparse=False):
        """v_sec, (Z, T) float64 F-order: the variance of the seconds of ONE trip that starts in zone o in hour t that comes from the
        truncated-normal draw alone, sum over d of p_destin[o, d, t] * var_sec(o, d, t), from the installed p_destin tables and the
        datamatrix.  Cached in the context until one of them changes (expected_trip_var_builds()).  sparse: from the compact rows of
        sparse tables (include/cpm_expected_sparse_var.h), in a cache of its own: the same bits where the means, the distances and
        var_sec of every cell that is not stored are finite."""
        v = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        call = self._L.cpm_expected_sparse_trip_var if sparse else self._L.cpm_expected_trip_var
        _lib.check(call(self._h, _vp(v)))
        return v

    def expected_trip_var_dev(self, d_v_ptr, sparse=False):
        """Enqueue on the context's stream: d_v_ptr = device address of float64[T][Z], v_sec.  sparse: as in expected_trip_var()."""
        call = self._L.cpm_expected_sparse_trip_var_dev if sparse else self._L.cpm_expected_trip_var_dev
        _lib.check(call(self._h, C.c_void_p(int(d_v_ptr)) if d_v_ptr else None))

    def expected_trip_var_builds(self, sparse=False):
        """How often this context has built the trip variance weights.  sparse: those of expected_trip_var(sparse=True), counted apart."""
        n = int((self._L.cpm_expected_sparse_trip_var_builds if sparse else self._L.cpm_expected_trip_var_builds)(self._h))
        if n < 0:
            _lib.check(n)
        return n

    def expected_travel_var(self, a_parking, b_driving, s_seconds=None, d_km=None, start=None, ivp=False, per_zone=False, sparse=False):
        """Exact mean and variance over the seed of
        L = sum(a_parking * parking) + sum(b_driving * driving) + sum over the trips of (s_seconds[o, t] * seconds + d_km[o, t] * km)
        of resample(travel=True), the trips counted at their origin o and hour t, given the cars' start zones, blocking: one backward
        pass over the p_destin tables, the datamatrix's means and the distance matrix.  The noise of the destination, of the
        travel-time draw and their covariance with where the car is afterwards are all in it.  s_seconds = 1 alone is the run's
        travel-time sum (sum_tt_q16 / 65536).  Coefficients: (Z, T), or (Z, T, K) for K functionals (at most CPM_MAX_BATCH);
        s_seconds / d_km None: zeros, and then every word is expected_linear_var()'s.  start, ivp, per_zone and the result: as in
        expected_linear_var().  sparse: from the compact rows of sparse tables (include/cpm_expected_sparse_var.h): the same bits under
        expected_trip_var(sparse=True)'s condition, the dense p_destin array neither read nor built."""
        a, b = np.asarray(a_parking, dtype=np.float64), np.asarray(b_driving, dtype=np.float64)
        sd = [None if x is None else np.asarray(x, dtype=np.float64) for x in (s_seconds, d_km)]
        single = a.ndim == 2
        if (a.ndim not in (2, 3) or a.shape[:2] != (self.Z, self.T) or (a.ndim == 3 and a.shape[2] < 1)
                or any(x.shape != a.shape for x in [b] + [x for x in sd if x is not None])):
            raise ValueError(f"expected_travel_var: coefficients {[x.shape for x in [a, b] + [x for x in sd if x is not None]]}, expected all of "
                             f"({self.Z}, {self.T}) or ({self.Z}, {self.T}, K)")
        K = 1 if single else a.shape[2]
        a, b = (np.asfortranarray(x.reshape(self.Z, self.T, K, order="F")) for x in (a, b))
        sd = [None if x is None else np.asfortranarray(x.reshape(self.Z, self.T, K, order="F")) for x in sd]
        w = None if start is None else np.ascontiguousarray(_f64(start, (self.Z,)))
        mean, var = np.zeros(K), np.zeros(K)
        zm = np.zeros((self.Z, K), order="F") if per_zone else None
        zv = np.zeros((self.Z, K), order="F") if per_zone else None
        call = self._L.cpm_expected_sparse_travel_var if sparse else self._L.cpm_expected_travel_var
        _lib.check(call(self._h, _vp(w), _lib.CPM_EXPECT_IVP if ivp else 0, K, _vp(a), _vp(b), _vp(sd[0]), _vp(sd[1]), _vp(mean), _vp(var), _vp(zm),
                        _vp(zv)))
        out = {"mean": float(mean[0]), "var": float(var[0])} if single else {"mean": mean, "var": var}
        if per_zone:
            out["zone_mean"], out["zone_var"] = (zm[:, 0], zv[:, 0]) if single else (zm, zv)
        return out

    def expected_travel_var_dev(self, K, d_coeff_ptr, d_out_ptr, d_start_ptr=0, ivp=False, d_zone_ptr=0, sparse=False):
        """Enqueue on the context's stream: d_coeff_ptr = device address of float64[K][4][T][Z] (A_k, B_k, S_k, D_k); d_out_ptr =
        device address of float64[K][2] (mean, variance); d_start_ptr = device address of float64[Z] or 0 (1 per zone); d_zone_ptr =
        device address of float64[K][2][Z] (per start zone) or 0.  sparse: as in expected_travel_var(); the coefficients must be
        finite (this call does not check them)."""
        p = lambda v: C.c_void_p(int(v)) if v else None
        call = self._L.cpm_expected_sparse_travel_var_dev if sparse else self._L.cpm_expected_travel_var_dev
        _lib.check(call(self._h, p(d_start_ptr), _lib.CPM_EXPECT_IVP if ivp else 0, int(K), p(d_coeff_ptr), p(d_out_ptr), p(d_zone_ptr)))

    def expected_batch_dev(self, d_out_ptr, d_pi0_ptr=0, ivp=False, sparse=False):
        """Enqueue on the context's stream: d_out_ptr = device address of float64[B][expected_words()] for the installed batch tables.
        sparse: cpm_expected_sparse_batch_dev, as in expected()."""
        call = self._L.cpm_expected_sparse_batch_dev if sparse else self._L.cpm_expected_batch_dev
        _lib.check(call(self._h, C.c_void_p(int(d_pi0_ptr)) if d_pi0_ptr else None, _lib.CPM_EXPECT_IVP if ivp else 0,
                        C.c_void_p(int(d_out_ptr)) if d_out_ptr else None))

    def expected_sparse_aux(self, sparse=True):
        """Test aid (cpm_expected_sparse_aux): (ell, r, start, list) of the installed tables as the sparse (True) or the dense builder
        left them: int32 (T, Z), float64 (T, Z), int32 (T, Z + 1), int32 (T, Z)."""
        ell = np.zeros((self.T, self.Z), dtype=np.int32)
        r = np.zeros((self.T, self.Z), dtype=np.float64)
        start = np.zeros((self.T, self.Z + 1), dtype=np.int32)
        lst = np.zeros((self.T, self.Z), dtype=np.int32)
        _lib.check(self._L.cpm_expected_sparse_aux(self._h, 1 if sparse else 0, _vp(ell), _vp(r), _vp(start), _vp(lst)))
        return ell, r, start, lst

    # -- expected travel time and distance (include/cpm_expected_travel.h): the trip weights of the tables, times the driving density --
    def expected_trip(self, sparse=False):
        """(w_sec, w_km), each (Z, T) float64 F-order: the expected seconds and kilometres of ONE trip that starts in zone o in hour
        t, from the installed p_destin tables, datamatrix and distance matrix alone.  Cached in the context until one of them changes.
        sparse: from the compact rows of sparse tables (include/cpm_expected_sparse_grad.h): the same bits where the means and
        distances are finite, the dense p_destin array neither read nor built; a cache of its own."""
        w_sec = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        w_km = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        call = self._L.cpm_expected_sparse_trip if sparse else self._L.cpm_expected_trip
        _lib.check(call(self._h, _vp(w_sec), _vp(w_km)))
        return w_sec, w_km

    def expected_trip_builds(self):
        """How often this context has built the trip weights."""
        n = int(self._L.cpm_expected_trip_builds(self._h))
        if n < 0:
            _lib.check(n)
        return n

    def expected_travel(self, pi0=None, ivp=False, sparse=False):
        """The expected travel of a fleet, blocking: dict(seconds, km: (Z, T) float64 F-order, the driving density of expected() times
        the trip weights; total_seconds, total_km; A_drive = total_seconds / (T * 3600), the noise-free share of the day a car
        drives).  C * seconds[z, t] is the expected travel-time sum of the cars that leave z in hour t of resample(travel=True).
        sparse: as in expected_trip(), its condition on the means and distances included; the propagation is expected(sparse=True)'s."""
        a = self._pi0(pi0)
        seconds = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        km = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        totals = np.zeros(2, dtype=np.float64)
        call = self._L.cpm_expected_sparse_travel if sparse else self._L.cpm_expected_travel
        _lib.check(call(self._h, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(seconds), _vp(km), _vp(totals)))
        return dict(seconds=seconds, km=km, total_seconds=float(totals[0]), total_km=float(totals[1]),
                    A_drive=float(totals[0]) / (self.T * 3600.0))

    def expected_travel_batch(self, pi0=None, ivp=False, sparse=False):
        """The same for every fleet of the installed batch tables: seconds, km (Z, T, B) and total_seconds, total_km, A_drive (B,);
        fleet b bit for bit expected_travel() with p_drive[:, :, b] installed.  sparse: as in expected_travel()."""
        a = self._pi0(pi0)
        B = self.get_info(_lib.CPM_INFO_BATCH)
        seconds = np.zeros((self.Z, self.T, B), dtype=np.float64, order="F")
        km = np.zeros((self.Z, self.T, B), dtype=np.float64, order="F")
        totals = np.zeros((B, 2), dtype=np.float64)
        call = self._L.cpm_expected_sparse_travel_batch if sparse else self._L.cpm_expected_travel_batch
        _lib.check(call(self._h, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(seconds), _vp(km), _vp(totals)))
        return dict(seconds=seconds, km=km, total_seconds=totals[:, 0].copy(), total_km=totals[:, 1].copy(),
                    A_drive=totals[:, 0] / (self.T * 3600.0))

    def expected_trip_dev(self, d_w_ptr, sparse=False):
        """Enqueue on the context's stream: d_w_ptr = device address of float64[2][T][Z], w_sec then w_km.  sparse: as in
        expected_trip()."""
        call = self._L.cpm_expected_sparse_trip_dev if sparse else self._L.cpm_expected_trip_dev
        _lib.check(call(self._h, C.c_void_p(int(d_w_ptr)) if d_w_ptr else None))

    def expected_travel_dev(self, d_expected_ptr, B, d_travel_ptr=0, d_totals_ptr=0, sparse=False):
        """Enqueue on the context's stream: d_expected_ptr = device address of float64[B][expected_words()] as expected_dev /
        expected_batch_dev wrote it (only the driving halves are read); d_travel_ptr = device address of float64[B][2][T][Z], seconds
        then km, or 0; d_totals_ptr = device address of float64[B][2] or 0.  Not both 0.  sparse: the weights of expected_trip(sparse=True)."""
        call = self._L.cpm_expected_sparse_travel_dev if sparse else self._L.cpm_expected_travel_dev
        _lib.check(call(self._h, C.c_void_p(int(d_expected_ptr)) if d_expected_ptr else None, int(B),
                        C.c_void_p(int(d_travel_ptr)) if d_travel_ptr else None, C.c_void_p(int(d_totals_ptr)) if d_totals_ptr else None))

    # -- the adjoint of the expected densities (include/cpm_expected_grad.h): gradients for p_drive and pi0 in one backward pass --
    def expected_grad(self, g_parking, g_driving, pi0=None, ivp=False, g_next=None, sparse=False):
        """The gradient of L = <g_parking, parking> + <g_driving, driving> + <g_next, pi_next> over expected()'s outputs at the installed
        tables, blocking: dict(grad_p_drive (Z, T) float64 F-order, grad_pi0 (Z,)).  g_parking / g_driving: (Z, T) cotangents, i.e. the
        derivative of an objective with respect to expected()'s densities; g_next: (Z,) or None (zeros).  grad_p_drive is exactly 0
        wherever the installed p_drive is not strictly inside (0, 1).  pi0, ivp: as for expected().  sparse: from the compact rows of sparse
        tables (include/cpm_expected_sparse_grad.h): the same bits for finite cotangents (this call checks them), the dense p_destin array
        neither read nor built."""
        a = self._pi0(pi0)
        gp = np.asfortranarray(_f64(g_parking, (self.Z, self.T)))
        gd = np.asfortranarray(_f64(g_driving, (self.Z, self.T)))
        gn = None if g_next is None else np.ascontiguousarray(_f64(g_next, (self.Z,)))
        grad = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        grad_pi0 = np.zeros(self.Z, dtype=np.float64)
        call = self._L.cpm_expected_sparse_grad if sparse else self._L.cpm_expected_grad
        _lib.check(call(self._h, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(gp), _vp(gd), _vp(gn), _vp(grad), _vp(grad_pi0)))
        return dict(grad_p_drive=grad, grad_pi0=grad_pi0)

    def expected_grad_dev(self, d_cotangent_ptr, d_grad_p_drive_ptr, d_pi0_ptr=0, ivp=False, d_gnext_ptr=0, d_grad_pi0_ptr=0, sparse=False):
        """Enqueue on the context's stream: d_cotangent_ptr = device address of float64[2][T][Z] (g_parking, then g_driving, laid out
        like expected_dev's tensor); d_grad_p_drive_ptr = device address of float64[T][Z]; d_pi0_ptr / d_gnext_ptr = device address of
        float64[Z] or 0 (uniform / zeros); d_grad_pi0_ptr = device address of float64[Z] or 0 (not wanted).  sparse: as in
        expected_grad(); the cotangents must be finite (the call does not check)."""
        p = lambda v: C.c_void_p(int(v)) if v else None
        call = self._L.cpm_expected_sparse_grad_dev if sparse else self._L.cpm_expected_grad_dev
        _lib.check(call(self._h, p(d_pi0_ptr), _lib.CPM_EXPECT_IVP if ivp else 0, p(d_cotangent_ptr), p(d_gnext_ptr), p(d_grad_p_drive_ptr),
                        p(d_grad_pi0_ptr)))

    # -- the adjoint along a tangent of p_destin (include/cpm_expected_grad_dest.h): the derivative for e_dest --
    def set_p_dest_tangent(self, dp, sparse=False):
        """Install a tangent of the p_destin tables: (Z, Z, T) float64 [origin, destination, hour], the layout of set_p_dest.  Every
        call that installs p_destin tables, and every new datamatrix, drops it.  sparse: onto the stored cells of sparse tables
        (include/cpm_expected_sparse_dest.h), hour by hour; the dense device array is not allocated, and a non-zero entry at a cell the
        rows do not store is refused.  The two tangents are independent of each other."""
        a = _f64(dp, (self.Z, self.Z, self.T))
        call = self._L.cpm_set_p_dest_tangent_sparse if sparse else self._L.cpm_set_p_dest_tangent
        _lib.check(call(self._h, _vp(a)))

    def build_p_dest_tangent(self, want=False, sparse=False):
        """d p_destin / d e_dest of the installed tables, built on the device from the resident datamatrix at the e_dest of the last
        build_p_dest (which must have installed the tables, with e_dest > 0).  want: also return it, (Z, Z, T) float64 F-order.
        sparse: the compact tangent on the stored cells, the same operations per cell; as in set_p_dest_tangent()."""
        if sparse:
            _lib.check(self._L.cpm_build_p_dest_tangent_sparse(self._h))
            return self.get_p_dest_tangent(sparse=True) if want else None
        out = np.zeros((self.Z, self.Z, self.T), dtype=np.float64, order="F") if want else None
        _lib.check(self._L.cpm_build_p_dest_tangent(self._h, _vp(out)))
        return out

    def get_p_dest_tangent(self, sparse=False):
        """The installed tangent, (Z, Z, T) float64 F-order.  sparse: the compact one, +0.0 off the stored cells."""
        out = np.zeros((self.Z, self.Z, self.T), dtype=np.float64, order="F")
        call = self._L.cpm_get_p_dest_tangent_sparse if sparse else self._L.cpm_get_p_dest_tangent
        _lib.check(call(self._h, _vp(out)))
        return out

    def expected_grad_dest(self, g_parking, g_driving, pi0=None, ivp=False, g_next=None, sparse=False):
        """expected_grad() with one more output: dict(grad_p_drive, grad_pi0, grad_dest (Z, T) float64 F-order).  grad_dest[o, t] is the
        derivative of L along the installed tangent restricted to row (o, t) of p_destin, the residual of the row held fixed;
        grad_dest.sum() is the derivative of L along the tangent.  grad_p_drive and grad_pi0 carry expected_grad()'s bits.  sparse: from
        the compact rows and the compact tangent (include/cpm_expected_sparse_dest.h): the same bits, neither dense array read or built."""
        a = self._pi0(pi0)
        gp = np.asfortranarray(_f64(g_parking, (self.Z, self.T)))
        gd = np.asfortranarray(_f64(g_driving, (self.Z, self.T)))
        gn = None if g_next is None else np.ascontiguousarray(_f64(g_next, (self.Z,)))
        grad = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        grad_pi0 = np.zeros(self.Z, dtype=np.float64)
        grad_dest = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        call = self._L.cpm_expected_sparse_grad_dest if sparse else self._L.cpm_expected_grad_dest
        _lib.check(call(self._h, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(gp), _vp(gd), _vp(gn), _vp(grad), _vp(grad_pi0), _vp(grad_dest)))
        return dict(grad_p_drive=grad, grad_pi0=grad_pi0, grad_dest=grad_dest)

    def expected_grad_dest_dev(self, d_cotangent_ptr, d_grad_p_drive_ptr, d_grad_dest_ptr, d_pi0_ptr=0, ivp=False, d_gnext_ptr=0, d_grad_pi0_ptr=0,
                               sparse=False):
        """Enqueue on the context's stream: the arguments of expected_grad_dev, and d_grad_dest_ptr = device address of float64[T][Z].
        sparse: as in expected_grad_dest()."""
        p = lambda v: C.c_void_p(int(v)) if v else None
        call = self._L.cpm_expected_sparse_grad_dest_dev if sparse else self._L.cpm_expected_grad_dest_dev
        _lib.check(call(self._h, p(d_pi0_ptr), _lib.CPM_EXPECT_IVP if ivp else 0, p(d_cotangent_ptr), p(d_gnext_ptr), p(d_grad_p_drive_ptr),
                        p(d_grad_pi0_ptr), p(d_grad_dest_ptr)))

    # -- the adjoint for the fleets of a batch (include/cpm_expected_grad_batch.h): B gradients in one pass over p_destin --
    @staticmethod
    def _sparse_dest(what, dest, sparse, compact_tangent):
        """The refusals of dest with sparse, before any device call: without compact_tangent the tangent is the dense array."""
        if compact_tangent and not sparse:
            raise ValueError(f"{what}: compact_tangent=True needs sparse=True: the dense calls read the dense tangent")
        if sparse and dest and not compact_tangent:
            raise ValueError(f"{what}: dest=True has no sparse form: the p_destin tangent is a dense array (compact_tangent=True reads the "
                             "compact one of build_p_dest_tangent(sparse=True))")

    def expected_grad_batch(self, g_parking, g_driving, pi0=None, ivp=False, g_next=None, dest=False, sparse=False, compact_tangent=False):
        """expected_grad() -- dest: expected_grad_dest() -- for every fleet of the installed batch tables, blocking.  g_parking /
        g_driving: (Z, T, B) cotangents, fleet b's in [:, :, b]; g_next: (Z, B) or None (zeros for all fleets); pi0 is shared.  Returns
        dict(grad_p_drive (Z, T, B) float64 F-order, grad_pi0 (Z, B)[, grad_dest (Z, T, B)]): fleet b's slices bit for bit what the
        B = 1 call returns with p_drive[:, :, b] installed and fleet b's cotangents.  sparse: as in expected_grad(); with dest only
        under compact_tangent=True, which reads the compact tangent (include/cpm_expected_sparse_dest.h) instead of the dense array."""
        Sampler._sparse_dest("expected_grad_batch", dest, sparse, compact_tangent)
        a = self._pi0(pi0)
        B = self.get_info(_lib.CPM_INFO_BATCH)
        if B < 1:  # (the library names what is missing; it reads no array before it does)
            B = np.asarray(g_parking).shape[-1] if np.asarray(g_parking).ndim == 3 else 1
        gp = np.asfortranarray(_f64(g_parking, (self.Z, self.T, B)))
        gd = np.asfortranarray(_f64(g_driving, (self.Z, self.T, B)))
        gn = None if g_next is None else np.asfortranarray(_f64(g_next, (self.Z, B)))
        grad = np.zeros((self.Z, self.T, B), dtype=np.float64, order="F")
        grad_pi0 = np.zeros((self.Z, B), dtype=np.float64, order="F")
        flags = _lib.CPM_EXPECT_IVP if ivp else 0
        if not dest:
            call = self._L.cpm_expected_sparse_grad_batch if sparse else self._L.cpm_expected_grad_batch
            _lib.check(call(self._h, _vp(a), flags, _vp(gp), _vp(gd), _vp(gn), _vp(grad), _vp(grad_pi0)))
            return dict(grad_p_drive=grad, grad_pi0=grad_pi0)
        grad_dest = np.zeros((self.Z, self.T, B), dtype=np.float64, order="F")
        call = self._L.cpm_expected_sparse_grad_dest_batch if sparse else self._L.cpm_expected_grad_dest_batch
        _lib.check(call(self._h, _vp(a), flags, _vp(gp), _vp(gd), _vp(gn), _vp(grad), _vp(grad_pi0), _vp(grad_dest)))
        return dict(grad_p_drive=grad, grad_pi0=grad_pi0, grad_dest=grad_dest)

    def expected_grad_batch_dev(self, d_cotangent_ptr, d_grad_p_drive_ptr, d_pi0_ptr=0, ivp=False, d_gnext_ptr=0, d_grad_pi0_ptr=0, sparse=False):
        """Enqueue on the context's stream: d_cotangent_ptr = device address of float64[B][2][T][Z] (laid out like expected_batch_dev's
        tensor); d_grad_p_drive_ptr = device address of float64[B][T][Z]; d_pi0_ptr = device address of float64[Z] or 0 (uniform);
        d_gnext_ptr / d_grad_pi0_ptr = device address of float64[B][Z] or 0 (zeros / not wanted).  sparse: as in expected_grad_dev()."""
        p = lambda v: C.c_void_p(int(v)) if v else None
        call = self._L.cpm_expected_sparse_grad_batch_dev if sparse else self._L.cpm_expected_grad_batch_dev
        _lib.check(call(self._h, p(d_pi0_ptr), _lib.CPM_EXPECT_IVP if ivp else 0, p(d_cotangent_ptr), p(d_gnext_ptr), p(d_grad_p_drive_ptr),
                        p(d_grad_pi0_ptr)))

    def expected_grad_dest_batch_dev(self, d_cotangent_ptr, d_grad_p_drive_ptr, d_grad_dest_ptr, d_pi0_ptr=0, ivp=False, d_gnext_ptr=0,
                                     d_grad_pi0_ptr=0, sparse=False):
        """Enqueue on the context's stream: the arguments of expected_grad_batch_dev, and d_grad_dest_ptr = device address of
        float64[B][T][Z].  sparse: as in expected_grad_dest()."""
        p = lambda v: C.c_void_p(int(v)) if v else None
        call = self._L.cpm_expected_sparse_grad_dest_batch_dev if sparse else self._L.cpm_expected_grad_dest_batch_dev
        _lib.check(call(self._h, p(d_pi0_ptr), _lib.CPM_EXPECT_IVP if ivp else 0, p(d_cotangent_ptr), p(d_gnext_ptr), p(d_grad_p_drive_ptr),
                        p(d_grad_pi0_ptr), p(d_grad_dest_ptr)))

    def expected_trip_tangent(self, sparse=False):
        """(dw_sec, dw_km), each (Z, T) float64 F-order: the derivative of expected_trip()'s weights along the installed tangent, the
        residual of every row held fixed.  sparse: along the compact tangent, from the stored cells (include/cpm_expected_sparse_dest.h)."""
        dw_sec = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        dw_km = np.zeros((self.Z, self.T), dtype=np.float64, order="F")
        call = self._L.cpm_expected_sparse_trip_tangent if sparse else self._L.cpm_expected_trip_tangent
        _lib.check(call(self._h, _vp(dw_sec), _vp(dw_km)))
        return dw_sec, dw_km

    def expected_trip_tangent_dev(self, d_dw_ptr, sparse=False):
        """Enqueue on the context's stream: d_dw_ptr = device address of float64[2][T][Z], dw_sec then dw_km.  sparse: as in
        expected_trip_tangent()."""
        call = self._L.cpm_expected_sparse_trip_tangent_dev if sparse else self._L.cpm_expected_trip_tangent_dev
        _lib.check(call(self._h, C.c_void_p(int(d_dw_ptr)) if d_dw_ptr else None))

    # -- value and four-parameter gradient of the noise-free objectives (include/cpm_expected_fit.h): one call, one forward pass --
    def set_measured_activity(self, activity):
        """The measured traffic activity, (T,), resident until replaced; None: forget it.  NaN or infinite entries raise."""
        if activity is None:
            _lib.check(self._L.cpm_set_measured_activity(self._h, None))
            return
        a = np.ascontiguousarray(_f64(activity, (self.T,)))
        _lib.check(self._L.cpm_set_measured_activity(self._h, _vp(a)))

    def fit_words(self):
        """float64 words of one fleet's expected_fit record: CPM_FIT_WORDS + T."""
        return _lib.CPM_FIT_WORDS + self.T

    def _fit_args(self, p_min, p_max, e_drive, weights):
        lo = np.ascontiguousarray(np.atleast_1d(np.asarray(p_min, dtype=np.float64)))
        B = lo.shape[0]
        hi = np.ascontiguousarray(_f64(np.atleast_1d(p_max), (B,)))
        ex = np.ascontiguousarray(_f64(np.atleast_1d(e_drive), (B,)))
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim == 1:
            w = np.broadcast_to(w, (B, 3))
        w = np.ascontiguousarray(_f64(w, (B, 3)))
        return B, lo, hi, ex, w

    def expected_fit_dev(self, p_min, p_max, e_drive, weights, d_record_ptr, d_pi0_ptr=0, ivp=False, dest=False, d_expected_ptr=0,
                         d_cotangent_ptr=0, d_grad_p_drive_ptr=0, d_grad_dest_ptr=0, sparse=False, compact_tangent=False):
        """Enqueue on the context's stream: the B points (p_min, p_max, e_drive: (B,)) with weights (B, 3) or (3,) = (w_act, w_park,
        w_adrive) into d_record_ptr = device address of float64[B][fit_words()].  The batch tables hold these points afterwards.
        d_expected_ptr / d_cotangent_ptr = device address of float64[B][2][T][Z] or 0; d_grad_p_drive_ptr / d_grad_dest_ptr = device
        address of float64[B][T][Z] or 0 (kept in the library's workspace).  dest: also dF/de_dest, along the installed tangent.
        sparse: from the compact rows of sparse tables (include/cpm_expected_sparse_grad.h): the same bits where every mean and distance
        at a cell that is not stored is finite (the dense trip weights form 0 * value there); with dest only under compact_tangent=True,
        which reads the compact tangent (include/cpm_expected_sparse_dest.h) instead of the dense array."""
        Sampler._sparse_dest("expected_fit_dev", dest, sparse, compact_tangent)
        B, lo, hi, ex, w = self._fit_args(p_min, p_max, e_drive, weights)
        p = lambda v: C.c_void_p(int(v)) if v else None
        flags = (_lib.CPM_EXPECT_IVP if ivp else 0) | (_lib.CPM_FIT_DEST if dest else 0)
        call = self._L.cpm_expected_sparse_fit_dev if sparse else self._L.cpm_expected_fit_dev
        _lib.check(call(self._h, B, _vp(lo), _vp(hi), _vp(ex), p(d_pi0_ptr), flags, _vp(w), p(d_record_ptr), p(d_expected_ptr), p(d_cotangent_ptr),
                        p(d_grad_p_drive_ptr), p(d_grad_dest_ptr)))

    @staticmethod
    def fit_record(rec, T):
        """An expected_fit record array (B, CPM_FIT_WORDS + T) as a dict of arrays over the fleets."""
        rec = np.asarray(rec, dtype=np.float64).reshape(-1, _lib.CPM_FIT_WORDS + T)
        names = ("F", "activity_error", "parking_error", "A_drive", "n_valid", "d_p_min", "d_p_max", "d_e_drive", "d_e_dest", "total_seconds",
                 "total_km")
        out = {k: rec[:, i].copy() for i, k in enumerate(names)}
        out["n_valid"] = out["n_valid"].astype(np.int64)
        out["traffic_activity"] = rec[:, _lib.CPM_FIT_WORDS:].copy()
        out["record"] = rec
        return out

    def expected_fit(self, p_min, p_max, e_drive, weights, pi0=None, ivp=False, dest=False, want=(), sparse=False, compact_tangent=False):
        """Value and gradient of F = w_act * activity_error + w_park * parking_error + w_adrive * A_drive at B points, blocking: a dict
        of (B,) arrays F, activity_error, parking_error, A_drive, n_valid, d_p_min, d_p_max, d_e_drive, d_e_dest (NaN without dest),
        total_seconds, total_km, traffic_activity (B, T) and record (B, fit_words()).  want: names among "expected", "cotangent" (each
        (B, 2, T, Z): parking then driving, hour-major), "grad_p_drive", "grad_dest" ((Z, T, B) F-order) to return as well.  sparse,
        compact_tangent: as in expected_fit_dev()."""
        Sampler._sparse_dest("expected_fit", dest, sparse, compact_tangent)
        unknown = set(want) - {"expected", "cotangent", "grad_p_drive", "grad_dest"}
        if unknown:
            raise ValueError(f"expected_fit: unknown outputs {sorted(unknown)}")
        if "grad_dest" in want and not dest:
            raise ValueError("expected_fit: grad_dest needs dest=True")
        B, lo, hi, ex, w = self._fit_args(p_min, p_max, e_drive, weights)
        a = self._pi0(pi0)
        rec = np.zeros((B, self.fit_words()), dtype=np.float64)
        arrs = {}
        for k in ("expected", "cotangent"):
            arrs[k] = np.zeros((B, 2, self.T, self.Z), dtype=np.float64) if k in want else None
        for k in ("grad_p_drive", "grad_dest"):
            arrs[k] = np.zeros((self.Z, self.T, B), dtype=np.float64, order="F") if k in want else None
        flags = (_lib.CPM_EXPECT_IVP if ivp else 0) | (_lib.CPM_FIT_DEST if dest else 0)
        call = self._L.cpm_expected_sparse_fit if sparse else self._L.cpm_expected_fit
        _lib.check(call(self._h, B, _vp(lo), _vp(hi), _vp(ex), _vp(a), flags, _vp(w), _vp(rec), _vp(arrs["expected"]), _vp(arrs["cotangent"]),
                        _vp(arrs["grad_p_drive"]), _vp(arrs["grad_dest"])))
        out = self.fit_record(rec, self.T)
        out.update({k: v for k, v in arrs.items() if v is not None})
        return out

    # -- the forward tangent of the expected densities (include/cpm_expected_tangent.h): K columns of the densities' Jacobian in one call --
    @staticmethod
    def _tangent_c(c_dest, K):
        return None if c_dest is None else np.ascontiguousarray(_f64(np.atleast_1d(c_dest), (K,)))

    def expected_tangent(self, K, d_p_drive=None, d_pi0=None, c_dest=None, pi0=None, ivp=False, want_next=False, want_expected=False,
                         sparse=False):
        """The derivative of expected()'s densities in K directions at the installed tables, blocking.  Direction k is
        (d_pi0[:, k], d_p_drive[:, :, k], c_dest[k] times the installed tangent of p_destin); d_p_drive: (Z, T, K), d_pi0: (Z, K),
        c_dest: (K,), each or None (zero).  Returns dict(d_parking, d_driving: (Z, T, K) float64 F-order[, d_pi_next (Z, K)][, parking,
        driving (Z, T): expected()'s bits]).  A direction of p_drive counts only where the installed p_drive is strictly inside (0, 1).
        sparse=True: the same bits from the compact rows and the compact tangent of sparse tables, neither dense array read, built or
        allocated (include/cpm_expected_sparse_tangent.h)."""
        K = int(K)
        n = max(K, 1)                              # (the library names a K out of range; it reads no array before it does)
        a = self._pi0(pi0)
        if 1 <= K <= _lib.CPM_TANGENT_MAX_DIRECTIONS:
            dpd = None if d_p_drive is None else _f64(d_p_drive, (self.Z, self.T, K))
            dp0 = None if d_pi0 is None else _f64(d_pi0, (self.Z, K))
            cd = self._tangent_c(c_dest, K)
        else:                                      # (whatever their shapes: CPM_ERR_ARG names K)
            dpd, dp0, cd = (None if v is None else np.asfortranarray(v, dtype=np.float64) for v in (d_p_drive, d_pi0, c_dest))
        d_parking = np.zeros((self.Z, self.T, n), dtype=np.float64, order="F")
        d_driving = np.zeros((self.Z, self.T, n), dtype=np.float64, order="F")
        nxt = np.zeros((self.Z, n), dtype=np.float64, order="F") if want_next else None
        parking = np.zeros((self.Z, self.T), dtype=np.float64, order="F") if want_expected else None
        driving = np.zeros((self.Z, self.T), dtype=np.float64, order="F") if want_expected else None
        call = self._L.cpm_expected_sparse_tangent if sparse else self._L.cpm_expected_tangent
        _lib.check(call(self._h, K, _vp(a), _lib.CPM_EXPECT_IVP if ivp else 0, _vp(dp0), _vp(dpd), _vp(cd), _vp(d_parking), _vp(d_driving), _vp(nxt),
                        _vp(parking), _vp(driving)))
        out = dict(d_parking=d_parking, d_driving=d_driving)
        if want_next:
            out["d_pi_next"] = nxt
        if want_expected:
            out.update(parking=parking, driving=driving)
        return out

    def expected_tangent_dev(self, K, d_out_ptr, d_dp_drive_ptr=0, d_dpi0_ptr=0, c_dest=None, d_pi0_ptr=0, ivp=False, d_dpi_next_ptr=0,
                             d_expected_ptr=0, flags=None, sparse=False):
        """Enqueue on the context's stream: d_out_ptr = device address of float64[K][2][T][Z] (per direction d parking, then d driving);
        d_dp_drive_ptr = device address of float64[K][T][Z] or 0, d_dpi0_ptr of float64[K][Z] or 0 (zero); c_dest: host (K,) or None;
        d_pi0_ptr = device address of float64[Z] or 0 (uniform); d_dpi_next_ptr = float64[K][Z] or 0; d_expected_ptr =
        float64[expected_words()] or 0 (the primal).  flags: the raw flag word in place of ivp.  sparse=True: from the compact rows
        and the compact tangent (include/cpm_expected_sparse_tangent.h)."""
        p = lambda v: C.c_void_p(int(v)) if v else None
        K = int(K)
        cd = self._tangent_c(c_dest, K) if 1 <= K <= _lib.CPM_TANGENT_MAX_DIRECTIONS else (
            None if c_dest is None else np.ascontiguousarray(c_dest, dtype=np.float64))   # (whatever its shape: CPM_ERR_ARG names K)
        f = (_lib.CPM_EXPECT_IVP if ivp else 0) if flags is None else int(flags)
        call = self._L.cpm_expected_sparse_tangent_dev if sparse else self._L.cpm_expected_tangent_dev
        _lib.check(call(self._h, K, p(d_pi0_ptr), f, p(d_dpi0_ptr), p(d_dp_drive_ptr), _vp(cd), p(d_out_ptr), p(d_dpi_next_ptr), p(d_expected_ptr)))

    def build_p_drive_tangent(self, p_min, p_max, e_drive):
        """d p_drive / d (p_min, p_max, e_drive) at the point, from the resident datamatrix: (Z, T, 3) float64 F-order, the direction
        tables of expected_tangent() for the three parameters.  The installed p_drive is not touched."""
        out = np.zeros((self.Z, self.T, 3), dtype=np.float64, order="F")
        _lib.check(self._L.cpm_build_p_drive_tangent(self._h, float(p_min), float(p_max), float(e_drive), _vp(out)))
        return out

    def build_p_drive_tangent_dev(self, p_min, p_max, e_drive, d_out_ptr):
        """Enqueue on the context's stream: d_out_ptr = device address of float64[3][T][Z]."""
        _lib.check(self._L.cpm_build_p_drive_tangent_dev(self._h, float(p_min), float(p_max), float(e_drive),
                                                         C.c_void_p(int(d_out_ptr)) if d_out_ptr else None))

    def last_kernel_ms(self):
        buf = (C.c_float * 8192)()
        n = C.c_int32(0)
        _lib.check(self._L.cpm_last_kernel_ms(self._h, C.cast(buf, C.c_void_p), 8192, C.byref(n)))
        return [float(buf[i]) for i in range(n.value)]

    def debug_categorical(self, origin, hour, k53):
        """Diagnostic: destinations (1-based; 0 = all-zero row) the grouped zone sampler draws from row
        (origin, hour) for the 53-bit uniforms k53 (u = k * 2^-53); also the number of exact-row fallbacks."""
        k = np.ascontiguousarray(k53, dtype=np.uint64)
        out = np.zeros(k.shape[0], dtype=np.int64)
        n_exact = C.c_int32(0)
        _lib.check(self._L.cpm_debug_categorical(self._h, int(origin), int(hour), int(k.shape[0]), _vp(k), _vp(out),
                                                 C.byref(n_exact)))
        return out, int(n_exact.value)

    def debug_travel_draw(self, k53, mean, sd):
        """Diagnostic: the travel kernels' truncated-normal draw, element by element, for cells (mean, sd) and the 53-bit uniforms k53
        (u = k * 2^-53): (draw float64, mass of the window float64, draw in 2^-16 s int64).  sd == 0 is a tenth of the mean, as in the
        kernels.  Needs no tables, datamatrix or cars."""
        k = np.ascontiguousarray(k53, dtype=np.uint64).reshape(-1)
        m = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        s = np.ascontiguousarray(sd, dtype=np.float64).reshape(-1)
        if not k.shape == m.shape == s.shape:
            raise ValueError(f"k53 {k.shape}, mean {m.shape} and sd {s.shape} must have one length")
        draw, mass, q = np.zeros(k.shape[0]), np.zeros(k.shape[0]), np.zeros(k.shape[0], dtype=np.int64)
        _lib.check(self._L.cpm_debug_travel_draw(self._h, int(k.shape[0]), _vp(k), _vp(m), _vp(s), _vp(draw), _vp(mass), _vp(q)))
        return draw, mass, q

    def debug_f64_kit(self, fn, x):
        """Diagnostic: fn(x) element by element through the sampler's deterministic f64 functions as the kernels are compiled; fn =
        _lib.CPM_KIT_LOG / _SQRT / _ERF / _PPND / _EXP_NEG, or its name ("log", "sqrt", "erf", "ppnd", "exp_neg")."""
        if isinstance(fn, str):
            fn = getattr(_lib, "CPM_KIT_" + fn.upper())
        a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        out = np.zeros(a.shape[0])
        _lib.check(self._L.cpm_debug_f64_kit(self._h, int(fn), int(a.shape[0]), _vp(a), _vp(out)))
        return out

    def algorithmic_bytes_per_hour(self):
        b = C.c_int64(0)
        _lib.check(self._L.cpm_algorithmic_bytes_per_hour(self._h, C.byref(b)))
        return int(b.value)


def flows_csr_to_dense(csr):
    """The (T, Z, Z) int32 tensor resample(flows=True) returns, from the dict of resample(flows="csr") (numpy only)."""
    T, Z, _ = csr["shape"]
    row_ptr = np.asarray(csr["row_ptr"], dtype=np.int64)
    out = np.zeros((T * Z, Z), dtype=np.int32)
    rows = np.repeat(np.arange(T * Z, dtype=np.int64), np.diff(row_ptr))
    out[rows, np.asarray(csr["dest"], dtype=np.int64)] = csr["count"]
    return out.reshape(T, Z, Z)


def flows_csr_hour(csr, t):
    """Hour t (0-based) of the dict of resample(flows="csr"): (indptr (Z + 1,) int64 rebased to 0, indices, data), the last two views,
    ready for scipy.sparse.csr_matrix((data, indices, indptr), shape=(Z, Z)) -- rows are origins, columns destinations."""
    T, Z, _ = csr["shape"]
    if not 0 <= t < T:
        raise IndexError(f"hour {t} of {T}")
    p = csr["row_ptr"][t * Z:(t + 1) * Z + 1]
    return p - p[0], csr["dest"][p[0]:p[-1]], csr["count"][p[0]:p[-1]]


def stay_length_histogram(stays, parked):
    """Stay lengths of a day over all zones, from the arrays of resample(stays=True) (numpy only): dict of three (T,) int64 arrays.
    completed[L]: stays of L whole hours with both ends inside the day (L < t); left_censored[L]: stays that began with the day and
    ended with a drive in hour L (L == t: at least L hours); open[h]: stays still open when the day ends, by hours parked so far
    (h = T - 1 - a: at least h hours)."""
    stays = np.asarray(stays)
    parked = np.asarray(parked)
    T = stays.shape[0]
    if stays.ndim != 3 or stays.shape[2] != T or parked.shape != (stays.shape[1], T):
        raise ValueError(f"stays {stays.shape} / parked {parked.shape}: expected (T, Z, T) and (Z, T)")
    by_hour = stays.sum(axis=1, dtype=np.int64)  # [t, L]
    left = np.diagonal(by_hour).copy()
    completed = np.tril(by_hour, -1).sum(axis=0)
    return dict(completed=completed, left_censored=left, open=parked.sum(axis=0, dtype=np.int64)[::-1].copy())


def paths_to_matrices(paths, zone0):
    """The reference's state_matrix ((n, T) int64, 1-based zones) and transition_matrix[:, :, 0:2] ((n, T, 2) float64: drove, 1-based
    destination) from the record of resample(paths=True) and zone0, the 1-based state the step started from (numpy only)."""
    paths = np.asarray(paths)
    zone0 = np.asarray(zone0, dtype=np.int64)
    if paths.ndim != 2 or zone0.shape != (paths.shape[1],):
        raise ValueError(f"paths {paths.shape} / zone0 {zone0.shape}: expected (T, n) and (n,)")
    T, n = paths.shape
    dest = (paths & np.uint32(0x7FFFFFFF)).astype(np.int64).T + 1          # (n, T)
    state = np.empty((n, T), dtype=np.int64)
    state[:, 0] = zone0
    state[:, 1:] = dest[:, :T - 1]
    trans = np.empty((n, T, 2), dtype=np.float64)
    trans[:, :, 0] = (paths >> np.uint32(31)).T
    trans[:, :, 1] = dest
    return state, trans


def paths_flows(paths, zone0, Z):
    """The (T, Z, Z) int32 OD trip counts resample(flows=True) returns, from the record of resample(paths=True) and zone0, the
    1-based state the step started from (numpy only): flows[t, o, d] = cars that drove from zone o + 1 to zone d + 1 in hour t."""
    state, trans = paths_to_matrices(paths, zone0)
    T = state.shape[1]
    flows = np.zeros((T, Z, Z), dtype=np.int32)
    for t in range(T):
        drove = trans[:, t, 0] == 1
        cell = (state[drove, t] - 1) * Z + (trans[drove, t, 1].astype(np.int64) - 1)
        flows[t] = np.bincount(cell, minlength=Z * Z).reshape(Z, Z)
    return flows


def parse_uber_csv(path):
    """The native CSV reader alone (host only): (n, 5) Fortran array = the reference's rawdata[:,1:5]."""
    L = _lib.load()
    n = C.c_int64(0)
    _lib.check(L.cpm_parse_uber_csv(os.fsencode(path), C.byref(n), None, 0))
    out = np.zeros((n.value, 5), dtype=np.float64, order="F")
    if n.value:
        _lib.check(L.cpm_parse_uber_csv(os.fsencode(path), C.byref(n), _vp(out), n.value))
    return out


def device_count():
    n = C.c_int32(0)
    _lib.check(_lib.load().cpm_device_count(C.byref(n)))
    return n.value


def device_info(device=0):
    name = C.create_string_buffer(256)
    cu = C.c_int32(0)
    mem = C.c_int64(0)
    _lib.check(_lib.load().cpm_device_info(device, name, 256, C.byref(cu), C.byref(mem)))
    return dict(name=name.value.decode(), cu_count=cu.value, hbm_bytes=mem.value)
