// cpm_api.hip -- host side of libcpm_hip.so: context, device memory, launches and the
// C ABI declared in include/cpm.h.  gfx950 only; there is no CPU path in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/cpm.h"
#include "../../include/cpm_flows.h"
#include "../../include/cpm_flows_csr.h"
#include "../../include/cpm_stays.h"
#include "../../include/cpm_paths.h"
#include "../../include/cpm_charge.h"
#include "../../include/cpm_objectives.h"
#include "../../include/cpm_expected.h"
#include "../../include/cpm_expected_travel.h"
#include "../../include/cpm_expected_grad.h"
#include "../../include/cpm_expected_grad_dest.h"
#include "../../include/cpm_expected_grad_batch.h"
#include "../../include/cpm_expected_fit.h"
#include "../../include/cpm_expected_tangent.h"
#include "../../include/cpm_expected_sparse_tangent.h"
#include "../../include/cpm_expected_sparse.h"
#include "../../include/cpm_expected_sparse_grad.h"
#include "../../include/cpm_expected_sparse_dest.h"
#include "../../include/cpm_expected_var.h"
#include "../../include/cpm_expected_linear_var.h"
#include "../../include/cpm_expected_travel_var.h"
#include "../../include/cpm_expected_sparse_var.h"
#include "cpm_kernels.h"
#include "cpm_flows.h"
#include "cpm_flows_csr.h"
#include "cpm_stays.h"
#include "cpm_paths.h"
#include "cpm_charge.h"
#include "cpm_tables.h"
#include "cpm_exact.h"
#include "cpm_grouped.h"
#include "cpm_batch.h"
#include "cpm_dataset.h"
#include "cpm_upload.h"
#include "cpm_ingest.h"
#include "cpm_kit_debug.h"
#include "cpm_objectives.h"
#include "cpm_expected.h"
#include "cpm_expected_travel.h"
#include "cpm_expected_grad.h"
#include "cpm_expected_grad_dest.h"
#include "cpm_expected_grad_batch.h"
#include "cpm_expected_fit.h"
#include "cpm_expected_tangent.h"
#include "cpm_expected_sparse_tangent.h"
#include "cpm_expected_sparse.h"
#include "cpm_expected_sparse_grad.h"
#include "cpm_expected_sparse_dest.h"
#include "cpm_expected_var.h"
#include "cpm_expected_linear_var.h"
#include "cpm_expected_travel_var.h"
#include "cpm_expected_sparse_var.h"
#include "cpm_buf.h"

static hipError_t ensure_stream(cpm_ctx *c);

namespace {

thread_local std::string g_last_error;

int32_t fail(int32_t code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? CPM_ERR_NOMEM : CPM_ERR_HIP, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                            \
    } while (0)

// Every entry that enqueues work: the context's device is current and the context has a stream (its own one is created on first
// need -- a HIP stream takes one of the process's few hardware queues when it is CREATED, GPU_MAX_HW_QUEUES = 4 by default, and
// streams beyond that share queues: two contexts that were each given a caller's stream before doing anything hold two queues and
// their resamples interleave on the chip; with two unused own streams in between they were measured to serialise).
#define CTX_TRY(ctx)                                                 \
    if (!(ctx)) return fail(CPM_ERR_ARG, "null context");            \
    HIP_TRY(hipSetDevice((ctx)->device));                            \
    HIP_TRY(ensure_stream(ctx))

template <typename T>
void dfree(T *&p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

// The owners of the context's allocations (cpm_buf.h): freed by their destructors, grown by reserve(), whose hipError_t goes through
// HIP_TRY like that of any other call.
struct DevAlloc {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinnedAlloc {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void free(void *p) { (void)hipHostFree(p); }
};
template <typename T>
using DevBuf = cpm::Buf<T, DevAlloc>;
template <typename T>
using PinnedBuf = cpm::Buf<T, PinnedAlloc>;

inline unsigned nblk(int64_t n, int b) { return static_cast<unsigned>((n + b - 1) / b); }

}  // namespace

struct cpm_ctx {
    int64_t Z = 0, T = 0;
    int Zp = 0;
    int device = 0;
    int cu_count = 0;
    hipStream_t own_stream = nullptr;  // created on first need (ensure_stream)
    hipStream_t stream = nullptr;      // what the context enqueues on: the caller's (cpm_set_stream) or own_stream
    bool have_stream = false;
    // tables
    // (d_pdrive / d_thr and d_last / d_ckpt are plain pointers, freed by cpm_destroy: FleetTable points the first two into the batch
    //  tables for a step and ensure_full_cdf nulls the other two around one launch -- an owner is never re-pointed)
    double *d_pdrive = nullptr;  // [T][Z]
    DevBuf<double> d_p;          // [T][Z dest][Z origin] p_destin as the reference lays it out (cpm_set_p_dest, cpm_build_p_dest, the synthetic
                                 // tables).  Resident: the row tables below are derived from it in one pass (k_build_rows), ties walk it
                                 // (search_exact_ckpt)
    DevBuf<double> d_cdf;        // [T][Z][Zp] canonical f64 CDF rows: built on first need (ensure_full_cdf) -- the car and exact-layout
    bool cdf_full = false;       // kernels and cpm_get_cdf_row read them, the grouped path never does
    DevBuf<uint32_t> d_hi;       // [T][Z][RW] row packs: guide + high words of the CDF (cpm_grouped.h)
    DevBuf<uint32_t> d_hin;      // [T][Z][narrow_row_words] the NARROW packs of dense tables (cpm_narrow.h), built from d_hi where the one-launch
    bool narrow_valid = false;   // hour will stream them (narrow_wanted); valid: they are d_hi's -- cleared by whatever writes d_hi (ensure_hi)
    int narrow_opt = 1;          // CPM_OPT_NARROW_PACK
    DevBuf<uint32_t> d_narrow_ties;  // [1] draws the narrow search resolved on the wide words, cumulative (CPM_INFO_NARROW_TIES)
    double *d_last = nullptr;    // [T][Z] row totals
    double *d_ckpt = nullptr;    // [T][nck][Z] every 32nd value of the running sums (exact fallback of the grouped path)
    long long *d_thr = nullptr;  // [T][Z] Bernoulli thresholds of p_drive (k_build_thr), rebuilt whenever p_drive changes
    int Zq = 0;
    DevBuf<double> d_dm;         // [2][T][Z][Z] (reference layout)
    DevBuf<double> d_dist;       // [Z][Z]
    DevBuf<double2> d_tt;             // [T][Z][Z] (mean, std) origin-major: what the grouped path's travel kernel gathers from (cpm_grouped.h)
    bool tt_valid = false;
    // the same as sparse rows (cpm_grouped.h, k_tts_*), when the largest row fits LDS: what the travel kernel stages per (origin, hour)
    DevBuf<uint2> d_tts_words;
    DevBuf<uint32_t> d_tts_off;
    DevBuf<cpm::TravelCell> d_tts_cells;
    size_t tts_lds = 0;
    bool tts_valid = false;
    bool tts_fixed = false;  // the travel rows are those of the compact dataset: fixed stride kDsCap, counts in d_ds_cnt
    // the current datamatrix as compact rows (cpm_dataset.h: ONE sweep of it; valid until it changes), when it is sparse enough
    DevBuf<cpm::DsCell> d_ds_cells;     // [T*Z][kDsCap] cells of every (hour, origin), sorted by destination
    DevBuf<uint32_t> d_ds_cnt;          // [T*Z] cells per row; then {longest row, a row outgrew its capacity}
    PinnedBuf<uint32_t> h_ds_stats;     // pinned twin of those two words
    bool ds_valid = false;              // the rows describe the current datamatrix (ds_ok: and are usable)
    bool ds_ok = false;
    int ds_max = 0;                     // longest row
    // ... and the p_destin tables built from them (k_ds_pdest): sparse packs in d_hi, what a tie walks in these three (owned by the
    // TABLE: they stay whole when the next dataset's cells arrive)
    DevBuf<double> d_sp;                // [T*Z][kDsCap] normalised p of every row's cells
    DevBuf<uint32_t> d_sj;              // ... their destinations
    DevBuf<uint32_t> d_scnt;            // [T*Z] cells per row
    bool sparse_tables = false;         // the installed p_destin tables are of that kind: d_p holds p_destin only when p_dense_valid
    bool p_dense_valid = false;
    bool tables_uploaded = false;       // ... or from an uploaded p_destin (cpm_upload.h, CPM_OPT_SPARSE_UPLOAD): the three arrays are all they come from
    bool sparse_upload = false;         // CPM_OPT_SPARSE_UPLOAD: cpm_set_p_dest tries the sparse route
    DevBuf<uint32_t> d_up_stats;        // {longest row, a row outgrew kDsCap} of k_up_compact, and their pinned twin
    PinnedBuf<uint32_t> h_up_stats;
    double tab_e_dest = 2.0;            // the exponent they were built with (cpm_refresh_tables)
    int tab_e_int = 1;
    int pk_G = 0, pk_Zc = 0;            // geometry of the packs in d_hi (with Zq): guide bits, entries in front of the pad
    DevBuf<double> d_pdrive_mean;     // [T][Z] mean_sum of createpdrive (src/createpdrive.jl:10-21): depends on datamatrix and dist only,
    bool pdrive_mean_valid = false;   // so the model-selection sweep (p_min, p_max, e_drive vary) computes it once
    bool have_pdrive = false, have_cdf = false, have_dmat = false, have_dist = false;
    bool have_dm() const { return have_dmat && have_dist; }
    // cars
    int64_t C_total = 0, cpz = 0, n = 0;
    cpm::CarIndex cars{0, 1};     // local car i = global car cars.begin + i * cars.stride
    DevBuf<uint32_t> d_zone0;     // [n] current zones
    DevBuf<uint32_t> d_ztmp;      // [n] ping-pong for the IVP
    DevBuf<uint32_t> d_rec;       // [T][n]
    DevBuf<int32_t> d_flows;      // [T][Z][Z] OD trip counts of the blocking cpm_resample_flows (allocated by its first call)
    // the same counts as compressed sparse rows (include/cpm_flows_csr.h): the blocking call's arrays, allocated by its first call
    DevBuf<int64_t> d_csr_row_ptr;     // [T*Z + 1]
    DevBuf<int32_t> d_csr_dest;        // [d_csr_dest.cap]
    DevBuf<int32_t> d_csr_count;       // ... as many
    int64_t csr_nnz = -1;              // what the last blocking call reported (-1: there was none)
    DevBuf<int32_t> d_flows_hour;      // [Z*Z + 4] one hour's dense block: how the per-car families reach the CSR form
    // parking stays (include/cpm_stays.h): the per-car side array of every stays call, and the blocking call's arrays
    DevBuf<uint32_t> d_stay_last;      // [>= n] since << 24 | zone (csrc/cpm_stays.h)
    DevBuf<int32_t> d_stays;           // [T][Z][T]
    DevBuf<int32_t> d_stay_parked;     // [Z][T]
    // charge (include/cpm_charge.h): the per-car side array of every charge call, and the blocking call's arrays
    DevBuf<uint2> d_ebat;              // [>= n] {since << 24 | zone, Wh} (csrc/cpm_charge.h)
    DevBuf<double> d_dist_rows;        // [Z][Z] the distance matrix origin-major, built on first use, stale wherever d_dist is replaced
    bool dist_rows_valid = false;
    DevBuf<int64_t> d_chg_load;        // [2][Z][T] charge | used
    DevBuf<int32_t> d_chg_short;       // [Z][T]
    DevBuf<uint32_t> d_chg_zone_power;     // [Z]
    DevBuf<uint32_t> d_chg_soc;        // [2][cap / 2] soc_in | soc_out
    // per-car day records (include/cpm_paths.h): the blocking call's array, kept from its first use, and the columns
    // cpm_paths_expand_dev writes where the caller wants no matrix
    DevBuf<uint32_t> d_paths;          // [T][n]
    DevBuf<char> d_expand_cols;        // [5][n] 8-byte words
    bool have_state = false;
    // results
    DevBuf<int64_t> d_counts;     // [2*T*Z + 2]
    PinnedBuf<int64_t> h_counts;  // pinned twin: the blocking calls bring the whole tensor (status word included) over in one copy
    DevBuf<int> d_err;
    PinnedBuf<int> h_err;         // pinned twin of the validation flag
    // zone-bucket paths
    cpm::ExactWork zx;
    cpm::GroupedWork zg;
    // AUTO moves from the grouped (fixed-stride) layout to the exact one after an overflow that growing the regions could not
    // absorb: the status word of every grouped step is copied to pinned host memory behind the step and looked at, without
    // waiting, when the next step is enqueued (the overflowed step itself is flagged in its own status word).
    bool grouped_overflowed = false;
    PinnedBuf<long long> h_status;      // pinned [2]: status word, largest heavy bucket of the step (GroupedWork::maxn)
    hipEvent_t status_ev = nullptr;
    bool status_pending = false;
    // An IVP enqueued on the grouped layout writes the new state beside the old one; it is committed (or repeated) by
    // finish_ivp() before anything reads or replaces the state or the tables.
    bool ivp_pending = false;
    uint64_t ivp_seed = 0;
    int ivp_form = -1;                  // the hour form of the pending IVP attempt (GroupedWork::last_form behind its grouped_run)
    cpm::LaunchCells ivp_cells;         // ... and what its launch helpers launched (GroupedWork::last_cells), likewise
    PinnedBuf<long long> h_ivp_status;  // pinned [2], likewise
    // what produced the results of the most recent step (CPM_INFO_LAST_KERNEL / _LAST_FORM), and the step attempts the library ran,
    // discarded and ran again so far (CPM_INFO_STEPS_REPEATED)
    int last_kernel = 0;
    int last_form = -1;
    int64_t steps_repeated = 0;
    int last_batch_fleets = 0;          // CPM_INFO_LAST_BATCH_FLEETS: 0 after every step that is not a batch step
    int last_hour = 0;                  // CPM_INFO_LAST_HOUR: 1 when hour T of the most recent step was a count-only launch (cpm_count.h)
    cpm::LaunchCells last_cells;        // CPM_INFO_CELL_*: the instantiations the most recent step launched, per role (all 0: none of these launchers ran)
    // batch tables and workspace (include/cpm_batch.h, cpm_batch.h)
    int batch_B = 0;
    DevBuf<double> d_pdrive_b;          // [B][T][Z] the fleets' p_drive tables
    DevBuf<long long> d_thr_b;          // [B][T][Z] their Bernoulli thresholds
    cpm::BatchWork zb;
    DevBuf<int64_t> d_bcounts;          // [B][2*T*Z + 2] the blocking batch call's count tensors, and their pinned twin
    PinnedBuf<int64_t> h_bcounts;
    // the asynchronous batch step's status words, ORed into one word and copied to pinned memory behind the step; looked at, without
    // waiting, when the next batch step is enqueued (as status_ev / h_status for the single path)
    DevBuf<unsigned long long> d_bstatus;
    PinnedBuf<unsigned long long> h_bstatus;
    hipEvent_t bstatus_ev = nullptr;
    bool bstatus_pending = false;
    // the sweep's objectives (include/cpm_objectives.h, cpm_objectives.h)
    DevBuf<double> d_measured;          // [T][Z] measured parking densities, and per zone whether its row sums to != 0
    DevBuf<int> d_meas_flag;            // [Z]
    bool have_measured = false;
    DevBuf<double> d_obj_part;          // [B][ceil(Z/256)] the workgroups' partial sums of the zone errors ...
    DevBuf<int> d_obj_part_n;           // ... and their counts of valid zones
    // expected densities (include/cpm_expected.h, cpm_expected.h): per-table arrays, built on first use and stale wherever d_last is rebuilt
    DevBuf<int> d_exp_ell;              // [T][Z] last destination with p > 0 (Z: a zero row)
    DevBuf<double> d_exp_r;             // [T][Z] max(0, 1 - last)
    DevBuf<int> d_exp_start;            // [T][Z + 1] where each destination's origins begin in ...
    DevBuf<int> d_exp_list;             // [T][Z] ... the origins sorted by (ell, origin)
    DevBuf<unsigned long long> d_exp_bad;     // the first row whose total exceeds 1, and its pinned twin
    PinnedBuf<unsigned long long> h_exp_bad;
    bool exp_aux_valid = false;
    // the same from the compact rows of sparse tables, and their transpose (include/cpm_expected_sparse.h, cpm_expected_sparse.h): arrays of
    // their own, so that exp_aux_valid keeps meaning "built with the dense array expanded"; stale wherever exp_aux_valid is
    DevBuf<int> d_exps_ell;             // [T][Z]
    DevBuf<double> d_exps_r;            // [T][Z]
    DevBuf<int> d_exps_start;           // [T][Z + 1]
    DevBuf<int> d_exps_list;            // [T][Z]
    DevBuf<uint32_t> d_exps_colptr;     // [T][Z + 1] where column (t, d) begins in ...
    DevBuf<uint32_t> d_exps_o;          // [cells] ... the origins and ...
    DevBuf<double> d_exps_p;            // [cells] ... the values of the stored cells, each column sorted by cpm::exps_key
    DevBuf<uint32_t> d_exps_cur;        // [T][Z + 1] the builder's counts, then its tickets
    DevBuf<unsigned long long> d_exps_stat;   // {first row whose total exceeds 1, cells}, and their pinned twin
    PinnedBuf<unsigned long long> h_exps_stat;
    size_t exps_cells = 0;
    bool exps_valid = false;
    DevBuf<double> d_exp_ws;            // [4][cap / 4] pi and x, ping and pong, of as many fleets ([Zs] each) as it was last grown for
    DevBuf<double> d_exp_out;           // [B][2][T][Z] + [Z] + [Z]: the blocking calls' outputs; pi_next and pi_0 end the allocation (exp_out_tail)
    // exact variances (include/cpm_expected_var.h, cpm_expected_var.h): allocated on first use
    DevBuf<double> d_var_p;             // [2][Z][Z] the transition matrix P_t, ping and pong
    DevBuf<double> d_var_part;          // [ceil(Z / 64)][4][Z] the start-row chunks' partial sums of one hour
    DevBuf<double> d_var_out;           // [4][T][Z] + [Z]: the blocking call's outputs, then its start weights
    // the variance of linear functionals (include/cpm_expected_linear_var.h, cpm_expected_linear_var.h): allocated on first use
    DevBuf<double> d_elv_ws;            // the passes' state [2][K4][2][Zs], the segments' sums [nseg][3][4][Zs], [K][2][Z] where the caller wants no d_zone
    DevBuf<double> d_elv_io;            // [K][2][T][Z] + [K][2] + [K][2][Z] + [Z]: the blocking call's coefficients, outputs, per-zone outputs and start weights
    // expected travel (include/cpm_expected_travel.h, cpm_expected_travel.h): the trip weights, built on first use and stale wherever
    // the p_destin tables (exp_aux_valid), d_dm or d_dist change
    DevBuf<double> d_exp_w;             // [2][T][Z] w_sec | w_km
    DevBuf<double> d_exp_wpart;         // [segments][2][T][Z] the destination segments' sums
    bool exp_trip_valid = false;
    int64_t exp_trip_builds = 0;
    // the trip variance weights (include/cpm_expected_travel_var.h, cpm_expected_travel_var.h): built behind the trip weights, and again
    // whenever those were rebuilt (exp_tvar_trip_build is the value of exp_trip_builds they were built at) -- one invalidation for both
    DevBuf<double> d_exp_vsec;          // [T][Z] v_sec
    int64_t exp_tvar_trip_build = 0;    // 0: never built
    int64_t exp_tvar_builds = 0;
    DevBuf<double> d_etv_ws;            // the passes' state [2][K2][2][Zs], the segments' sums [nseg][3][2][Zs], [K][2][Z] where the caller wants no d_zone
    DevBuf<double> d_etv_io;            // [K][4][T][Z] + [K][2] + [K][2][Z] + [Z]: the blocking call's coefficients, outputs, per-zone outputs and start weights
    // ... and the same weights from the compact rows (include/cpm_expected_sparse_grad.h): a cache of their own, so that a sparse call
    // never changes what a later dense call returns; stale wherever exp_trip_valid or exps_valid is
    DevBuf<double> d_exps_w;            // [2][T][Z] w_sec | w_km
    bool exps_trip_valid = false;
    DevBuf<double> d_exp_trav;          // [B][2][T][Z] + [B][2]: the blocking calls' seconds | km and totals, B = cap / (2 T Z + 2)
    DevBuf<double> d_exp_tpart;         // [B][chunks][2] the chunks' sums of k_exp_travel, added in order by k_exp_travel_total
    // the adjoint of the expected densities (include/cpm_expected_grad.h, cpm_expected_grad.h)
    DevBuf<double> d_exp_gws;           // [N + 4 + segments][Zs]: pi_s of the N = 2T - 1 operators, x ping and pong, mu ping and pong, the segments' sums
    DevBuf<double> d_exp_gio;           // [2][T][Z] + [Z] + [T][Z] + [Z] + [Z]: the blocking call's cotangents, G_next, grad_p_drive, grad_pi0 and pi_0
    // the adjoint along a tangent of p_destin (include/cpm_expected_grad_dest.h, cpm_expected_grad_dest.h)
    DevBuf<double> d_tan;               // [T][Z dest][Z origin] the tangent table, allocated by the first call that installs one
    bool tan_valid = false;             // ... and whether it belongs to the installed p_destin tables (dropped by every call that installs them)
    bool dest_built = false;            // the installed p_destin came from cpm_build_p_dest on the datamatrix still resident, at ...
    double dest_built_e = 0.0;          // ... this exponent
    int dest_built_int = 0;
    DevBuf<double> d_tan_m;             // [T][Z] the rows' sums of p * log(x) of the dense builder
    DevBuf<double> d_tan_w;             // [2][T][Z] the blocking trip-tangent call's dw_sec | dw_km
    DevBuf<double> d_exp_gdio;          // [T][Z] the blocking call's grad_dest
    int64_t tan_gen = 0;                // tangent tables installed so far: what a cached trip-weight tangent is checked against
    // ... and the same tangent on the stored cells of sparse tables (include/cpm_expected_sparse_dest.h, cpm_expected_sparse_dest.h):
    // independent of d_tan, dropped wherever tan_valid is
    DevBuf<double> d_sdp;               // [T * Z][kDsCap] entry for entry with d_sp, allocated by the first call that installs one
    bool sdp_valid = false;
    int64_t sdp_gen = 0;                // compact tangents installed so far
    DevBuf<double> d_sdp_stage;         // [Z dest][Z origin] one hour of a host tangent on its way to or from the cells; released after the call
    DevBuf<unsigned long long> d_sdp_bad;   // the first non-zero entry of a host tangent off the stored cells, and its pinned twin
    PinnedBuf<unsigned long long> h_sdp_bad;
    DevBuf<double> d_fits_dw;           // [2][T][Z] the trip weights' tangent of the sparse fit, kept while sdp and the sparse trip weights stay
    int64_t fits_dw_gen = -1, fits_dw_builds = -1;
    int64_t exps_trip_builds = 0;       // builds of d_exps_w so far
    // ... and the trip variance weights from the compact rows (include/cpm_expected_sparse_var.h): a cache of their own behind d_exps_w,
    // as d_exp_vsec is behind d_exp_w (exps_tvar_trip_build is the value of exps_trip_builds they were built at)
    DevBuf<double> d_exps_vsec;         // [T][Z] v_sec
    int64_t exps_tvar_trip_build = 0;   // 0: never built
    int64_t exps_tvar_builds = 0;
    // ... and carried into the transposed cell order for the forward tangent (include/cpm_expected_sparse_tangent.h): beside d_exps_o /
    // d_exps_p, built by the first tangent call with a non-zero c_dest, stale wherever sdp_gen moves or ensure_exps rebuilds
    DevBuf<double> d_exps_dp;           // [exps_cells]
    int64_t exps_dp_gen = -1;           // the sdp_gen it was built from (-1: none)
    // value and gradient of the noise-free objectives (include/cpm_expected_fit.h, cpm_expected_fit.h)
    DevBuf<double> d_act_meas;          // [T] measured traffic activity
    bool have_act_meas = false;
    DevBuf<double> d_fit_ws;            // the call's workspace: densities, cotangents, gradients and the O(B * (T + Z)) words (expected_fit_enqueue)
    DevBuf<int> d_fit_int;              // [B][Z] the zones' argmin | argmax, [B][ceil(Z/256)] the workgroups' counts of valid zones
    DevBuf<double> d_fit_dw;            // [2][T][Z] the trip weights' tangent, kept while the tangent table and the trip weights stay
    int64_t fit_dw_gen = -1, fit_dw_builds = -1;
    DevBuf<double> d_fit_rec;           // [B][CPM_FIT_WORDS + T] the blocking call's records
    // forward tangent of the expected densities (include/cpm_expected_tangent.h, cpm_expected_tangent.h)
    DevBuf<double> d_tanf_ws;           // [2][passes][2][8][Zs] pi | x of the passes' vectors, ping and pong; [2][Zs] xm; [Zs] u (expected_tangent_enqueue)
    DevBuf<double> d_tanf_io;           // the blocking calls' pi_0, directions and outputs (expected_tangent_blocking), or the builder's [3][T][Z]
    // options
    int kernel = CPM_KERNEL_AUTO;
    bool profile = false;
    int prof_what = CPM_PROFILE_SAMPLER;  // CPM_OPT_PROFILE_KERNEL
    int64_t fused_bailouts = 0;           // steps that came back with status bit 2 (a block of a one-launch form gave up waiting)
    int prof_stride = 1;      // bracket every prof_stride-th hourly sampler launch
    int64_t prof_seen = 0;    // sampler launches since profiling was switched on
    bool prof_open = false;
    std::vector<hipEvent_t> ev;  // 2 per hourly launch
    int n_prof = 0;
};

static hipError_t ensure_stream(cpm_ctx *c)
{
    if (c->have_stream) return hipSuccess;
    if (!c->own_stream) {
        hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
    }
    c->stream = c->own_stream;
    c->have_stream = true;
    return hipSuccess;
}


namespace {

// Every call that installs p_destin tables, and every new datamatrix: the tangent table no longer belongs to the tables, and they
// no longer come from cpm_build_p_dest on the resident datamatrix (cpm_build_p_dest says so again when it has succeeded).
void drop_dest_tangent(cpm_ctx *c)
{
    c->tan_valid = false;
    c->sdp_valid = false;
    c->dest_built = false;
}

int32_t ensure_cars(cpm_ctx *c, int64_t n)
{
    if (n == c->n && c->d_zone0) return CPM_OK;
    c->d_zone0.release();  // (exact-size, not grow-only: a smaller fleet gives the memory back, the per-car record with it)
    c->d_ztmp.release();
    c->d_rec.release();
    c->n = n;
    if (n > 0) {
        HIP_TRY(c->d_zone0.reserve(static_cast<size_t>(n)));
        HIP_TRY(c->d_ztmp.reserve(static_cast<size_t>(n)));
    }
    return CPM_OK;
}

int32_t ensure_rec(cpm_ctx *c)
{
    HIP_TRY(c->d_rec.reserve(static_cast<size_t>(c->n * c->T)));
    return CPM_OK;
}

int32_t check_err_flag(cpm_ctx *c, const char *what, int32_t code)
{
    // (into pinned memory: a copy into pageable memory goes through the runtime's staging path -- ~1 ms per call, measured on createpdestin)
    HIP_TRY(hipMemcpyAsync(c->h_err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int h = *c->h_err;
    if (h) {
        HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
        return fail(code, "%s", what);
    }
    return CPM_OK;
}

// the integer Bernoulli thresholds of the p_drive now in d_pdrive (enqueued on the context's stream)
int32_t update_thr(cpm_ctx *c)
{
    const int64_t n = c->Z * c->T;
    if (!c->d_thr) HIP_TRY(hipMalloc(&c->d_thr, sizeof(long long) * static_cast<size_t>(n)));
    hipLaunchKernelGGL(cpm::k_build_thr, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->d_pdrive, c->d_thr, n);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

int32_t ensure_narrow(cpm_ctx *c);

template <bool CDF, bool PACK>
hipError_t launch_build_rows(cpm_ctx *c)
{
    const hipError_t e = cpm::lds_opt_in<cpm::k_build_rows<CDF, PACK>>(cpm::kRowLds);  // (two 64 x 65 f64 tiles)
    if (e != hipSuccess) return e;
    dim3 grid(nblk(c->Z, cpm::kRowTile), static_cast<unsigned>(c->T));
    hipLaunchKernelGGL((cpm::k_build_rows<CDF, PACK>), grid, dim3(cpm::kRowBlock), cpm::kRowLds, c->stream, c->d_p, CDF ? c->d_cdf.get() : nullptr,
                       PACK ? c->d_hi.get() : nullptr, c->d_last, c->d_ckpt, static_cast<int>(c->Z), c->Zp, cpm::pack_zq(static_cast<int>(c->Z)),
                       cpm::pack_guide_bits(static_cast<int>(c->Z)), c->d_err);
    return hipGetLastError();
}

// Every writer of the row packs asks for them here: the narrow packs derived from them are stale from this moment on.
int32_t ensure_hi(cpm_ctx *c, size_t words)
{
    c->narrow_valid = false;
    HIP_TRY(c->d_hi.reserve(words));
    return CPM_OK;
}

// The table in d_p -> everything the samplers read: row totals, checkpoints and -- when a row pack fits LDS -- the row packs
// of the grouped path, in one pass.  The f64 CDF rows are built with them only when no pack fits (then every kernel searches f64
// rows) or when the caller asks; otherwise on first need (ensure_full_cdf).
int32_t build_rows(cpm_ctx *c, bool with_cdf)
{
    const int64_t rows = c->T * c->Z;
    const bool pack = cpm::pack_row_fits(static_cast<int>(c->Z));
    const bool cdf = with_cdf || !pack;
    c->have_cdf = false;
    c->exp_aux_valid = false;
    c->exps_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    c->cdf_full = false;
    if (!c->d_last) HIP_TRY(hipMalloc(&c->d_last, sizeof(double) * static_cast<size_t>(rows)));
    if (!c->d_ckpt) HIP_TRY(hipMalloc(&c->d_ckpt, sizeof(double) * static_cast<size_t>(rows) * cpm::ckpt_count(static_cast<int>(c->Z))));
    c->sparse_tables = false;  // (dense packs of the table in d_p)
    c->tables_uploaded = false;
    c->p_dense_valid = true;
    c->Zq = cpm::pack_zq(static_cast<int>(c->Z));
    c->pk_G = cpm::pack_guide_bits(static_cast<int>(c->Z));
    c->pk_Zc = static_cast<int>(c->Z);
    if (pack) {
        int32_t rc_hi = ensure_hi(c, static_cast<size_t>(rows) * cpm::pack_row_words(c->Zq, c->pk_G));
        if (rc_hi != CPM_OK) return rc_hi;
    }
    if (cdf) HIP_TRY(c->d_cdf.reserve(static_cast<size_t>(rows) * c->Zp));
    hipError_t e_rows;
    if (cdf && pack) e_rows = launch_build_rows<true, true>(c);
    else if (cdf) e_rows = launch_build_rows<true, false>(c);
    else e_rows = launch_build_rows<false, true>(c);
    HIP_TRY(e_rows);
    int32_t rc = check_err_flag(c, "p_dest holds NaN or negative entries (reference: BoundsError, Appendix A-7)", CPM_ERR_TABLE);
    if (rc != CPM_OK) return rc;
    c->have_cdf = true;
    c->cdf_full = cdf;
    return ensure_narrow(c);  // (every path that installs dense packs ends here: synth_tables, build_p_dest, set_p_dest, refresh_tables)
}

// p_destin in the reference's layout when the installed tables came from a compact dataset (cpm_dataset.h): only for what reads it --
// a caller that wants the array, the kernels that search f64 rows
int32_t ensure_dense_p(cpm_ctx *c)
{
    if (!c->sparse_tables || c->p_dense_valid) return CPM_OK;
    const size_t bytes = sizeof(double) * c->Z * c->Z * c->T;
    HIP_TRY(c->d_p.reserve(bytes / sizeof(double)));
    HIP_TRY(hipMemsetAsync(c->d_p, 0, bytes, c->stream));
    hipLaunchKernelGGL(cpm::k_ds_dense_p, dim3(cpm::ds_grid(c->T * c->Z)), dim3(cpm::kDsThreads * cpm::kDsRows), 0, c->stream, c->d_sp, c->d_sj, c->d_scnt,
                       cpm::kDsCap, c->T * c->Z, static_cast<int>(c->Z), c->d_p);
    HIP_TRY(hipGetLastError());
    c->p_dense_valid = true;
    return CPM_OK;
}

// the canonical f64 CDF rows of the installed table, for the kernels that search them (enqueued on the context's stream)
int32_t ensure_full_cdf(cpm_ctx *c)
{
    if (c->cdf_full) return CPM_OK;
    if (!c->have_cdf) return fail(CPM_ERR_STATE, "p_dest not set");
    {
        int32_t rc_p = ensure_dense_p(c);
        if (rc_p != CPM_OK) return rc_p;
    }
    HIP_TRY(c->d_cdf.reserve(static_cast<size_t>(c->T * c->Z) * c->Zp));
    double *keep_last = c->d_last, *keep_ckpt = c->d_ckpt;  // (already built: this pass writes the CDF rows only)
    c->d_last = nullptr;
    c->d_ckpt = nullptr;
    hipError_t e = launch_build_rows<true, false>(c);
    c->d_last = keep_last;
    c->d_ckpt = keep_ckpt;
    HIP_TRY(e);
    c->cdf_full = true;
    return CPM_OK;
}

bool grouped_fits(const cpm_ctx *c, int cap_mult)
{
    return c->d_hi && c->d_last && (c->d_ckpt || c->sparse_tables) && c->d_thr && cpm::grouped_path_fits(c->n, static_cast<int>(c->Z), cap_mult);
}

// AUTO: a zone-bucketed LDS path when a row fits in LDS and there are enough cars per zone to amortise streaming every row once
// per hour (the grouped fixed-stride form while no overflow went unabsorbed in this context, else the exact layout); otherwise
// one thread per car.
int pick_kernel(const cpm_ctx *c)
{
    if (c->kernel != CPM_KERNEL_AUTO) return c->kernel;
    if (c->n >= 32 * c->Z && c->n < (int64_t(1) << 30)) {
        if (!c->grouped_overflowed && grouped_fits(c, c->zg.cap_mult)) return CPM_KERNEL_ZONE_GROUPED;
        if (cpm::exact_path_fits(static_cast<int>(c->Z))) return CPM_KERNEL_ZONE_LDS;
    }
    return CPM_KERNEL_CAR;
}

// After an overflow of the grouped layout: twice the bucket regions (and runs), while the problem still fits; the next
// enqueue re-allocates the workspace.  false: no room to grow -- the caller falls back to the exact layout for good.
bool grow_grouped(cpm_ctx *c)
{
    const int next = c->zg.cap_mult * 2;
    if (next > cpm::kMaxCapMult || !grouped_fits(c, next)) return false;
    c->zg.cap_mult = next;
    c->zg.buckets0_valid = false;
    return true;
}

// CPM_INFO_FUSED: the one-launch form the next grouped step takes (0: two launches per hour)
int fused_form(const cpm_ctx *c)
{
    // (the conditions grouped_run decides on: the day launch needs two applied hours and bucket regions below the counters' XCD
    //  bits; with one hour a run has no hour to fuse but in the placing-first form)
    const bool day = c->zg.fused_day && c->T >= 3 && cpm::grouped_cap(c->n, static_cast<int>(c->Z), c->zg.cap_mult) < (1u << cpm::kCntXccShift);
    return (pick_kernel(c) == CPM_KERNEL_ZONE_GROUPED && c->zg.fused_ok && c->zg.parts <= 1 &&
            cpm::fused_shape_ok(static_cast<int>(c->Z), c->Zq, c->pk_G, c->sparse_tables) &&
            (!c->zg.fused_auto || cpm::fused_pays(static_cast<int>(c->Z), c->Zq, c->pk_G, c->cu_count, c->sparse_tables, (c->n + c->Z - 1) / std::max<int64_t>(c->Z, 1))))
               ? (day ? 6 : (c->zg.fused_pf ? 3 : (c->T >= 2 ? 1 : 0)))
               : 0;
}

// The next grouped step would stream narrow packs (cpm_narrow.h): asked for, dense packs installed, and the rule says they pay.
bool narrow_wanted(const cpm_ctx *c)
{
    return c->narrow_opt != 0 && c->have_cdf && c->d_hi && c->n > 0 &&
           cpm::narrow_pays(static_cast<int>(c->Z), !c->sparse_tables, fused_form(c) == 1, c->zg.use_perm != 1, c->zg.fused_auto);
}

// The narrow packs of the installed dense packs, where the context will use them: at the end of every install, and in front of a grouped
// step (an option, the cars or the form may have changed since).  Where the rule says no, nothing is built.
int32_t ensure_narrow(cpm_ctx *c)
{
    if (c->narrow_valid || !narrow_wanted(c)) return CPM_OK;
    const int64_t rows = c->T * c->Z;
    HIP_TRY(c->d_hin.reserve(static_cast<size_t>(rows) * cpm::narrow_row_words(c->Zq, c->pk_G)));
    if (!c->d_narrow_ties) {
        HIP_TRY(c->d_narrow_ties.reserve(1));
        HIP_TRY(hipMemsetAsync(c->d_narrow_ties, 0, sizeof(uint32_t), c->stream));
    }
    HIP_TRY(cpm::narrow_build_rows(c->d_hi, c->d_hin, rows, static_cast<int>(c->Z), c->Zq, c->pk_G, c->stream));
    c->narrow_valid = true;
    return CPM_OK;
}

cpm::GroupedTables grouped_tables(const cpm_ctx *c)
{
    cpm::GroupedTables tb;
    tb.rp = c->d_hi;
    if (c->narrow_valid && narrow_wanted(c)) {
        tb.rpn = c->d_hin;
        tb.narrow_ties = c->d_narrow_ties;
    }
    tb.last = c->d_last;
    tb.thr = c->d_thr;
    tb.ckpt = c->d_ckpt;
    tb.p = c->d_p;
    tb.tt = c->d_tt;
    if (c->tts_valid) {
        tb.tts_words = c->d_tts_words;
        tb.tts_off = c->d_tts_off;
        tb.tts_cells = c->d_tts_cells;
        tb.tts_W = static_cast<int>((c->Z + 31) / 32);
        tb.tts_lds = c->tts_lds;
    }
    if (c->tts_valid && c->tts_fixed) {  // (travel rows of a compact dataset: fixed stride, counts beside them)
        tb.tts_cnt = c->d_ds_cnt;
        tb.tts_stride = cpm::kDsCap;
    }
    tb.Z = static_cast<int>(c->Z);
    tb.Zp = c->Zp;
    tb.Zq = c->Zq;
    tb.T = static_cast<int>(c->T);
    tb.G = c->pk_G;
    tb.Zc = c->pk_Zc;
    tb.smap = c->sparse_tables ? 1 : 0;
    if (c->sparse_tables) {
        tb.sp = c->d_sp;
        tb.sj = c->d_sj;
        tb.scnt = c->d_scnt;
        tb.scap = cpm::kDsCap;
    }
    return tb;
}

constexpr int kMaxProf = 8192;

void prof_begin(cpm_ctx *c, int what = CPM_PROFILE_SAMPLER)
{
    if (what != c->prof_what) return;
    c->prof_open = false;
    if (!c->profile || c->n_prof >= kMaxProf) return;
    if ((c->prof_seen++ % c->prof_stride) != 0) return;  // every prof_stride-th launch of the kind
    size_t k = static_cast<size_t>(c->n_prof) * 2;
    while (c->ev.size() < k + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;  // (no pair: this launch is not timed, nothing is counted)
        c->ev.push_back(e);
    }
    cpm::launch_timer() = cpm::LaunchTimer{c->ev[k], c->ev[k + 1]};  // carried by the launch that follows (cpm::launch)
    c->prof_open = true;                                               // only now: the pair exists and the timer is armed
}

void prof_end(cpm_ctx *c, int what = CPM_PROFILE_SAMPLER)
{
    if (what != c->prof_what || !c->prof_open) return;
    c->prof_open = false;
    const bool taken = cpm::launch_timer().start == nullptr;  // cpm::launch clears the timer when it hands the pair to a dispatch
    cpm::launch_timer() = cpm::LaunchTimer{};
    if (taken) c->n_prof++;  // a pair no launch stamped is reused by the next timed launch, never read
}

// one hourly step of the one-thread-per-car kernel
int32_t launch_step_car(cpm_ctx *c, const uint32_t *zin, uint32_t *out, int t, uint32_t step, uint64_t seed,
                        bool travel, unsigned long long *tt_sum)
{
    const double *pd = c->d_pdrive + static_cast<size_t>(t) * c->Z;
    const double *cdf = c->d_cdf + static_cast<size_t>(t) * c->Z * c->Zp;
    dim3 grid(nblk(c->n, 256)), block(256);
    if (travel)
        cpm::launch(cpm::k_step_car<true>, grid, block, 0, c->stream, zin, out, pd, cdf, static_cast<int>(c->Z),
                           c->Zp, c->n, c->cars, step, seed, c->d_dm.get(), static_cast<int>(c->T), t, tt_sum);
    else
        cpm::launch(cpm::k_step_car<false>, grid, block, 0, c->stream, zin, out, pd, cdf, static_cast<int>(c->Z),
                           c->Zp, c->n, c->cars, step, seed, nullptr, static_cast<int>(c->T), t, nullptr);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

int32_t launch_histogram(cpm_ctx *c, int64_t *d_counts)
{
    unsigned long long *parking = reinterpret_cast<unsigned long long *>(d_counts);
    unsigned long long *driving = parking + c->T * c->Z;
    size_t lds = sizeof(uint32_t) * 2 * c->Z;
    if (lds <= 160 * 1024) {
        HIP_TRY(cpm::lds_opt_in<cpm::k_histogram>(lds));
        // enough chunks to fill the chip, few enough that the flush (2*Z atomics per block) stays small
        int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((c->n + 16383) / 16384, 2 * c->cu_count / std::max<int64_t>(c->T / 4, 1) + 8));
        int64_t chunk = (c->n + chunks - 1) / chunks;
        dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(c->T));
        hipLaunchKernelGGL(cpm::k_histogram, grid, dim3(1024), lds, c->stream, c->d_zone0, c->d_rec, c->n,
                           static_cast<int>(c->Z), parking, driving, chunk);
    } else {
        dim3 grid(nblk(c->n, 256), static_cast<unsigned>(c->T));
        hipLaunchKernelGGL(cpm::k_histogram_global, grid, dim3(256), 0, c->stream, c->d_zone0, c->d_rec, c->n,
                           static_cast<int>(c->Z), parking, driving);
    }
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

int32_t finish_ivp(cpm_ctx *c);

// The current datamatrix as compact rows (cpm_dataset.h), once per datamatrix: ONE sweep of it (k_ds_cells), then the rows sorted and
// the travel rows written from them (k_ds_sort).  ds_ok: every row fits its capacity and the sparse pack of the longest row is at most
// 60 % of the dense one -- else the dense builders of cpm_tables.h / cpm_grouped.h take the dataset, as they take every T != 24.
int32_t ensure_dataset(cpm_ctx *c)
{
    if (c->ds_valid) return CPM_OK;
    c->ds_ok = false;
    if (!cpm::ds_fits(c->Z, c->T) || !cpm::pack_row_fits(static_cast<int>(c->Z))) {
        c->ds_valid = true;
        return CPM_OK;
    }
    const int64_t rows = c->T * c->Z;
    const int W = static_cast<int>((c->Z + 31) / 32);
    HIP_TRY(c->d_ds_cells.reserve(static_cast<size_t>(rows) * cpm::kDsCap));
    HIP_TRY(c->d_ds_cnt.reserve(static_cast<size_t>(rows + 2)));
    HIP_TRY(c->h_ds_stats.reserve(2));
    HIP_TRY(hipMemsetAsync(c->d_ds_cnt, 0, sizeof(uint32_t) * static_cast<size_t>(rows + 2), c->stream));
    hipLaunchKernelGGL(cpm::k_ds_cells, dim3(nblk(c->Z, 64), nblk(c->Z, cpm::kDsJB)), dim3(256), 0, c->stream, c->d_dm, c->d_ds_cells, c->d_ds_cnt,
                       static_cast<int>(c->Z), cpm::kDsCap, c->d_ds_cnt + rows);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_ds_stats, c->d_ds_cnt + rows, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ds_max = static_cast<int>(std::max<uint32_t>(c->h_ds_stats[0], 1u));
    c->ds_valid = true;
    const int zq_c = cpm::pack_zq(c->ds_max), g_c = cpm::pack_guide_bits(c->ds_max);
    const int dense_words = cpm::pack_row_words(cpm::pack_zq(static_cast<int>(c->Z)), cpm::pack_guide_bits(static_cast<int>(c->Z)));
    if (c->h_ds_stats[1] != 0 || 10 * cpm::pack_row_words(zq_c, g_c, 1) > 6 * dense_words) return CPM_OK;  // dense: the builders of cpm_tables.h
    HIP_TRY(c->d_tts_words.reserve(static_cast<size_t>(rows) * W));
    HIP_TRY(c->d_tts_cells.reserve(static_cast<size_t>(rows) * cpm::kDsCap));
    const size_t lds_sort = sizeof(uint32_t) * 2 * W * cpm::kDsRows;
    hipLaunchKernelGGL(cpm::k_ds_sort, dim3(cpm::ds_grid(rows)), dim3(cpm::kDsThreads * cpm::kDsRows), lds_sort, c->stream, c->d_ds_cells, c->d_ds_cnt, cpm::kDsCap,
                       rows, static_cast<int>(c->Z), c->d_tts_words, W, c->d_tts_cells);
    HIP_TRY(hipGetLastError());
    c->ds_ok = true;
    // the travel rows of this datamatrix are those just written: bitmap words + the longest row's cells must fit the travel kernel's LDS
    const size_t lds = ((static_cast<size_t>(W) * sizeof(uint2) + 15) & ~static_cast<size_t>(15)) + static_cast<size_t>(c->ds_max) * sizeof(cpm::TravelCell);
    if (lds <= 32 * 1024) {
        c->tts_lds = lds;
        c->tts_valid = true;
        c->tts_fixed = true;
        c->tt_valid = true;
        c->d_tt.release();  // (a dense table left over from a datamatrix whose rows did not fit)
    }
    return CPM_OK;
}

// createpdestin on the compact rows (k_ds_pdest): sparse packs, row totals and what a tie walks; false when this dataset / exponent
// takes the dense builders (x^0 = 1 also where x = 0: every cell of the dense table then holds weight)
int32_t build_p_dest_sparse(cpm_ctx *c, double e_dest, int32_t e_is_integer, bool *done)
{
    *done = false;
    if (!(e_dest > 0.0)) return CPM_OK;
    int32_t rc = ensure_dataset(c);
    if (rc != CPM_OK || !c->ds_ok) return rc;
    const int64_t rows = c->T * c->Z;
    const int nc = c->ds_max, zq_c = cpm::pack_zq(nc), g_c = cpm::pack_guide_bits(nc);
    HIP_TRY(c->d_sp.reserve(static_cast<size_t>(rows) * cpm::kDsCap));
    HIP_TRY(c->d_sj.reserve(static_cast<size_t>(rows) * cpm::kDsCap));
    HIP_TRY(c->d_scnt.reserve(static_cast<size_t>(rows)));
    if (!c->d_last) HIP_TRY(hipMalloc(&c->d_last, sizeof(double) * static_cast<size_t>(rows)));
    rc = ensure_hi(c, static_cast<size_t>(rows) * cpm::pack_row_words(zq_c, g_c, 1));
    if (rc != CPM_OK) return rc;
    c->have_cdf = false;
    c->cdf_full = false;
    c->exp_aux_valid = false;
    c->exps_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    hipLaunchKernelGGL(cpm::k_ds_pdest, dim3(cpm::ds_grid(rows)), dim3(cpm::kDsThreads * cpm::kDsRows), 0, c->stream, c->d_ds_cells, c->d_ds_cnt, cpm::kDsCap,
                       rows, static_cast<int>(c->Z), e_dest, e_is_integer, nc, zq_c, g_c, c->d_hi, c->d_last, c->d_sp, c->d_sj, c->d_scnt, c->d_err);
    HIP_TRY(hipGetLastError());
    c->sparse_tables = true;
    c->tables_uploaded = false;
    c->p_dense_valid = false;
    c->Zq = zq_c;
    c->pk_G = g_c;
    c->pk_Zc = nc;
    c->tab_e_dest = e_dest;
    c->tab_e_int = e_is_integer;
    rc = check_err_flag(c, "p_dest holds NaN or negative entries (reference: BoundsError, Appendix A-7)", CPM_ERR_TABLE);
    if (rc != CPM_OK) return rc;
    c->have_cdf = true;
    *done = true;
    return CPM_OK;
}

// The sparse packs of an uploaded table from its compact rows in d_sp / d_sj / d_scnt (k_up_pack): what cpm_set_p_dest ends in on the
// sparse route and what cpm_refresh_tables re-runs.  nc = the longest row.  Enqueued on the context's stream.
int32_t pack_uploaded_rows(cpm_ctx *c, int nc)
{
    const int64_t rows = c->T * c->Z;
    const int zq_c = cpm::pack_zq(nc), g_c = cpm::pack_guide_bits(nc);
    c->exp_aux_valid = false;
    c->exps_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    if (!c->d_last) HIP_TRY(hipMalloc(&c->d_last, sizeof(double) * static_cast<size_t>(rows)));
    int32_t rc = ensure_hi(c, static_cast<size_t>(rows) * cpm::pack_row_words(zq_c, g_c, 1));
    if (rc != CPM_OK) return rc;
    prof_begin(c, CPM_PROFILE_UPLOAD);
    cpm::launch(cpm::k_up_pack, dim3(cpm::ds_grid(rows)), dim3(cpm::kDsThreads * cpm::kDsRows), 0, c->stream, c->d_sp.get(), c->d_sj.get(), c->d_scnt.get(),
                cpm::kDsCap, rows, nc, zq_c, g_c, c->d_hi.get(), c->d_last);
    prof_end(c, CPM_PROFILE_UPLOAD);
    HIP_TRY(hipGetLastError());
    c->Zq = zq_c;
    c->pk_G = g_c;
    c->pk_Zc = nc;
    return CPM_OK;
}

// cpm_set_p_dest with CPM_OPT_SPARSE_UPLOAD: the array just copied into d_p -> compact rows (k_up_compact) -> sparse packs, under the
// dataset route's own rule (ensure_dataset): a row pack fits LDS, no row holds more than kDsCap non-zero entries, and the sparse pack
// of the longest row is at most 60 % of the dense one.  *done = false: the table does not qualify and the caller builds dense packs.
// The dense copy stays valid in d_p: the f64-row kernels, cpm_get_cdf_row and ties' readers see the bytes that were uploaded.
int32_t upload_p_dest_sparse(cpm_ctx *c, bool *done)
{
    *done = false;
    if (!cpm::pack_row_fits(static_cast<int>(c->Z))) return CPM_OK;
    const int64_t rows = c->T * c->Z;
    HIP_TRY(c->d_sp.reserve(static_cast<size_t>(rows) * cpm::kDsCap));
    HIP_TRY(c->d_sj.reserve(static_cast<size_t>(rows) * cpm::kDsCap));
    HIP_TRY(c->d_scnt.reserve(static_cast<size_t>(rows)));
    HIP_TRY(c->d_up_stats.reserve(2));
    HIP_TRY(c->h_up_stats.reserve(2));
    c->sparse_tables = false;  // (the compact rows of whatever table was installed are gone from here on)
    c->tables_uploaded = false;
    HIP_TRY(hipMemsetAsync(c->d_up_stats, 0, 2 * sizeof(uint32_t), c->stream));
    prof_begin(c, CPM_PROFILE_UPLOAD);
    cpm::launch(cpm::k_up_compact, dim3(nblk(c->Z, 64), static_cast<unsigned>(c->T)), dim3(64), 0, c->stream, c->d_p.get(), c->d_sp.get(), c->d_sj.get(),
                c->d_scnt.get(), static_cast<int>(c->Z), cpm::kDsCap, c->d_up_stats.get(), c->d_err.get());
    prof_end(c, CPM_PROFILE_UPLOAD);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_up_stats, c->d_up_stats, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    int32_t rc = check_err_flag(c, "p_dest holds NaN or negative entries (reference: BoundsError, Appendix A-7)", CPM_ERR_TABLE);  // (synchronises)
    if (rc != CPM_OK) return rc;
    const int nc = static_cast<int>(std::max<uint32_t>(c->h_up_stats[0], 1u));
    const int dense_words = cpm::pack_row_words(cpm::pack_zq(static_cast<int>(c->Z)), cpm::pack_guide_bits(static_cast<int>(c->Z)));
    if (c->h_up_stats[1] != 0 || nc > static_cast<int>(cpm::kDsCap) ||
        10 * cpm::pack_row_words(cpm::pack_zq(nc), cpm::pack_guide_bits(nc), 1) > 6 * dense_words)
        return CPM_OK;  // dense packs: build_rows
    c->cdf_full = false;
    rc = pack_uploaded_rows(c, nc);
    if (rc != CPM_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sparse_tables = true;
    c->tables_uploaded = true;
    c->p_dense_valid = true;
    c->have_cdf = true;
    *done = true;
    return CPM_OK;
}

// The travel table as sparse rows (once per datamatrix, straight from it): kept when the largest row -- its bitmap words
// and its non-zero cells -- fits 32 KB of LDS; the travel kernel then stages an origin's row instead of gathering cells from HBM.
int32_t build_sparse_travel_rows(cpm_ctx *c)
{
    c->tts_valid = false;
    c->tts_fixed = false;
    const int64_t rows = c->T * c->Z;
    const int W = static_cast<int>((c->Z + 31) / 32);
    HIP_TRY(c->d_tts_words.reserve(static_cast<size_t>(rows) * W));
    HIP_TRY(c->d_tts_off.reserve(static_cast<size_t>(rows + 1)));
    DevBuf<uint32_t> d_count;  // (scratch of this call: the rows' counts, then the largest of them)
    HIP_TRY(d_count.reserve(static_cast<size_t>(rows) + 4));
    uint32_t *d_max = d_count + rows;
    DevBuf<unsigned long long> d_total;
    HIP_TRY(d_total.reserve(1));
    const dim3 tgrid(nblk(c->Z, 64), static_cast<unsigned>(c->T), cpm::kTtsSplit);
    hipLaunchKernelGGL(cpm::k_tts_bits, tgrid, dim3(64), 0, c->stream, c->d_dm, c->d_tts_words, static_cast<int>(c->Z), static_cast<int>(c->T), W);
    hipLaunchKernelGGL(cpm::k_tts_prefix, dim3(nblk(rows, 256)), dim3(256), 0, c->stream, c->d_tts_words, d_count, rows, W);
    hipLaunchKernelGGL(cpm::k_tts_offsets, dim3(1), dim3(1024), 0, c->stream, d_count, c->d_tts_off, rows, d_max, d_total);
    HIP_TRY(hipGetLastError());
    uint32_t h_max = 0;
    unsigned long long h_total = 0;
    HIP_TRY(hipMemcpyAsync(&h_max, d_max, sizeof h_max, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&h_total, d_total, sizeof h_total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t lds = ((static_cast<size_t>(W) * sizeof(uint2) + 15) & ~static_cast<size_t>(15)) + static_cast<size_t>(h_max) * sizeof(cpm::TravelCell);
    if (lds > 32 * 1024 || h_total >= (1ull << 32)) return CPM_OK;  // dense rows: the travel kernel gathers from the dense table
    HIP_TRY(c->d_tts_cells.reserve(h_total));
    hipLaunchKernelGGL(cpm::k_tts_cells, tgrid, dim3(64), 0, c->stream, c->d_dm, c->d_tts_words, c->d_tts_off, c->d_tts_cells,
                       static_cast<int>(c->Z), static_cast<int>(c->T), W);
    HIP_TRY(hipGetLastError());
    c->tts_lds = lds;
    c->tts_valid = true;
    c->d_tt.release();  // (a dense table left over from a datamatrix whose rows did not fit)
    return CPM_OK;
}

// What a non-zero status word of a grouped step asks of the context.  Bit 2 (4): a placing block of the fused hour gave up waiting
// for its sampler workgroups (a dispatch order the hand-off did not expect): two launches per hour from now on.  Bit 1 (2): a bucket
// region or a run overflowed: twice the regions while the problem still fits.  true: the step can be repeated on the grouped path.
bool absorb_status(cpm_ctx *c, long long st)
{
    const bool bailed = (st & 4) != 0;
    if (bailed && c->zg.fused_ok) {
        c->zg.fused_ok = false;
        ++c->fused_bailouts;  // (CPM_INFO_FUSED_BAILOUTS: the context has left the one-launch forms for good)
    }
    // (a step that bailed out AND overflowed: the two-launch path is tried on the regions as they are when they cannot grow)
    const bool grown = (st & ~4ll) != 0 && grow_grouped(c);
    return bailed || grown;
}

// The travel tables of the grouped path's travel kernel, once per datamatrix: the travel rows of its compact rows (cpm_dataset.h) ...
int32_t ensure_travel_tables(cpm_ctx *c)
{
    if (!c->tt_valid) {
        int32_t rc_ds = ensure_dataset(c);
        if (rc_ds != CPM_OK) return rc_ds;
    }
    if (!c->tt_valid) {  // ... or, datasets those do not take: sparse rows for LDS, or -- rows too large -- the dense table
        int32_t rc_tts = build_sparse_travel_rows(c);
        if (rc_tts != CPM_OK) return rc_tts;
        if (!c->tts_valid) {
            const size_t cells = static_cast<size_t>(c->Z) * c->Z * c->T;
            HIP_TRY(c->d_tt.reserve(cells));
            hipLaunchKernelGGL(cpm::k_build_travel_table, dim3(nblk(c->Z, cpm::kTtTile), nblk(c->Z, cpm::kTtTile), static_cast<unsigned>(c->T)),
                               dim3(cpm::kTtTile * 8), 0, c->stream, c->d_dm, c->d_tt, static_cast<int>(c->Z), static_cast<int>(c->T));
            HIP_TRY(hipGetLastError());
        }
        c->tt_valid = true;
    }
    return CPM_OK;
}

// side (cpm_runs.h): where the side outputs of the step go, from whatever family produces the counts.  flows: the OD trip counts --
// nowhere, DEVICE int32[T][Z][Z] (cpm_flows.h) or DEVICE CSR arrays (cpm_flows_csr.h).  stays: the parking stays (cpm_stays.h) -- nowhere,
// or DEVICE int32[T][Z][T] + int32[Z][T] (stays.last is the context's own side array, set here).  paths: the per-car record of the day
// (cpm_paths.h) -- nowhere, or DEVICE uint32[T][n], every word of which is written by whatever family runs
int32_t resample_enqueue(cpm_ctx *c, uint64_t seed, uint32_t flags, int64_t *d_counts, cpm::SideDest side = cpm::SideDest{})
{
    cpm::FlowsDest &fd = side.flows;
    cpm::StaysDest &sd = side.stays;
    const cpm::PathsDest &pd = side.paths;
    cpm::ChargeDest &cd = side.charge;
    int32_t *const d_flows = fd.dense;
    if (sd.any() && c->T > cpm::kStaysMaxT) return fail(CPM_ERR_ARG, "stays: T = %lld, the per-car word keeps an hour in 8 bits (T <= %d)", (long long)c->T, cpm::kStaysMaxT);
    if (sd.any() && c->Z > static_cast<int64_t>(cpm::kStayZoneMask)) return fail(CPM_ERR_ARG, "stays: Z = %lld, the per-car word keeps a zone in 24 bits", (long long)c->Z);
    if (cd.any() && c->T > cpm::kStaysMaxT) return fail(CPM_ERR_ARG, "charge: T = %lld, the per-car word keeps an hour in 8 bits (T <= %d)", (long long)c->T, cpm::kStaysMaxT);
    if (cd.any() && c->Z > static_cast<int64_t>(cpm::kStayZoneMask)) return fail(CPM_ERR_ARG, "charge: Z = %lld, the per-car word keeps a zone in 24 bits", (long long)c->Z);
    if (cd.any() && !c->have_dist) return fail(CPM_ERR_STATE, "charge: no distance matrix (cpm_set_datamatrix with dist, cpm_set_distance or cpm_set_distance_from_centroids)");
    if (!c->have_pdrive || !c->have_cdf) return fail(CPM_ERR_STATE, "resample: p_drive / p_dest not set");
    if (!c->have_state) return fail(CPM_ERR_STATE, "resample: no car state (cpm_init_states / cpm_set_state)");
    {
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    bool travel = (flags & CPM_FLAG_TRAVEL) != 0;
    if (travel && !c->have_dm()) return fail(CPM_ERR_STATE, "CPM_FLAG_TRAVEL needs cpm_set_datamatrix");
    size_t nwords = static_cast<size_t>(2 * c->T * c->Z + 2);
    if (c->status_pending && hipEventQuery(c->status_ev) == hipSuccess) {
        c->status_pending = false;
        if (c->h_status[0] != 0 && !absorb_status(c, c->h_status[0])) c->grouped_overflowed = true;
        c->zg.set_parts(static_cast<uint32_t>(c->h_status[1]), static_cast<uint32_t>(c->h_status[1] >> 32));
    }
    const int kernel = pick_kernel(c);
    c->last_kernel = kernel;  // (the family this call enqueues; the grouped path's form is recorded behind its run)
    c->last_batch_fleets = 0;
    c->last_hour = 0;
    c->last_cells = cpm::LaunchCells{};
    c->last_form = kernel == CPM_KERNEL_ZONE_GROUPED ? 0 : -1;
    if (c->n == 0 || kernel != CPM_KERNEL_ZONE_GROUPED)  // (the grouped path zeroes the count tensor with its other counters, in one launch)
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * nwords, c->stream));
    if (d_flows && (c->n == 0 || kernel != CPM_KERNEL_ZONE_GROUPED))  // (k_flows_cars adds to it; k_grouped_flows writes every row itself)
        HIP_TRY(hipMemsetAsync(d_flows, 0, sizeof(int32_t) * static_cast<size_t>(c->T) * c->Z * c->Z, c->stream));
    if (fd.csr() && c->n == 0)  // (no car, no trip: every row is empty)
        HIP_TRY(hipMemsetAsync(fd.row_ptr, 0, sizeof(int64_t) * (static_cast<size_t>(c->T) * c->Z + 1), c->stream));
    if (sd.any()) {  // (k_stays_parked adds to `parked` in every family, k_stays_cars to `stays`; k_grouped_stays writes every row itself)
        HIP_TRY(hipMemsetAsync(sd.parked, 0, sizeof(int32_t) * static_cast<size_t>(c->Z) * c->T, c->stream));
        if (c->n == 0 || kernel != CPM_KERNEL_ZONE_GROUPED)
            HIP_TRY(hipMemsetAsync(sd.stays, 0, sizeof(int32_t) * static_cast<size_t>(c->T) * c->Z * c->T, c->stream));
    }
    if (cd.any()) {  // (k_charge_cars adds to `used` and `short`, k_grouped_charge writes every word itself; `charge` is zeroed by k_charge_init)
        const size_t zt = static_cast<size_t>(c->Z) * c->T;
        if (c->n == 0) HIP_TRY(hipMemsetAsync(cd.charge, 0, sizeof(int64_t) * zt, c->stream));
        if (c->n == 0 || kernel != CPM_KERNEL_ZONE_GROUPED) {
            HIP_TRY(hipMemsetAsync(cd.used, 0, sizeof(int64_t) * zt, c->stream));
            HIP_TRY(hipMemsetAsync(cd.shrt, 0, sizeof(int32_t) * zt, c->stream));
        }
    }
    if (c->n == 0) return CPM_OK;
    if (cd.any()) {  // the side array: every car where the day began with its initial charge, at the start of every attempt
        HIP_TRY(c->d_ebat.reserve(static_cast<size_t>(c->n)));
        cd.ebat = c->d_ebat;
        // the origin's distances: a row of the context's origin-major copy of the distance matrix, built once per matrix
        HIP_TRY(c->d_dist_rows.reserve(static_cast<size_t>(c->Z) * c->Z));
        if (!c->dist_rows_valid) HIP_TRY(cpm::charge_launch_dist_rows(c->stream, c->d_dist, static_cast<int>(c->Z), c->d_dist_rows));
        c->dist_rows_valid = true;
        cd.dist = c->d_dist_rows;
        HIP_TRY(cpm::charge_launch_init(c->stream, c->d_zone0, c->n, static_cast<int>(c->Z), static_cast<int>(c->T), cd));
    }
    if (sd.any()) {  // the side array: every car "here since the day began", at the start of every attempt
        HIP_TRY(c->d_stay_last.reserve(static_cast<size_t>(c->n)));
        sd.last = c->d_stay_last;
        HIP_TRY(hipMemsetAsync(sd.last, 0, sizeof(uint32_t) * static_cast<size_t>(c->n), c->stream));
    }
    // the stays still open at the end of the day: behind the last hour of whichever family ran
    auto parked_pass = [&](int32_t rc_run) -> int32_t {
        if (rc_run != CPM_OK) return rc_run;
        if (sd.any()) HIP_TRY(cpm::stays_launch_parked(c->stream, c->d_zone0, c->n, static_cast<int>(c->Z), static_cast<int>(c->T), sd));
        if (cd.any()) HIP_TRY(cpm::charge_launch_close(c->stream, c->n, static_cast<int>(c->Z), static_cast<int>(c->T), cd));  // (and the charging of the stays still open)
        return CPM_OK;
    };
    if (fd.csr() && kernel != CPM_KERNEL_ZONE_GROUPED) {  // (k_flows_cars adds to a dense hour block, k_flows_csr_from_dense takes it apart)
        HIP_TRY(c->d_flows_hour.reserve(static_cast<size_t>(c->Z) * c->Z + 4));
        fd.hour_block = c->d_flows_hour;
    }
    unsigned long long *tt_sum = reinterpret_cast<unsigned long long *>(d_counts) + 2 * c->T * c->Z;
    if (kernel == CPM_KERNEL_ZONE_GROUPED) {
        if (!grouped_fits(c, c->zg.cap_mult))
            return fail(CPM_ERR_ARG, "CPM_KERNEL_ZONE_GROUPED does not fit this problem (use CPM_KERNEL_ZONE_LDS or CPM_KERNEL_CAR)");
        if (travel) {
            int32_t rc_tt = ensure_travel_tables(c);
            if (rc_tt != CPM_OK) return rc_tt;
        }
        {
            int32_t rc_n = ensure_narrow(c);
            if (rc_n != CPM_OK) return rc_n;
        }
        int32_t rc = cpm::grouped_run(c->zg, c->stream, grouped_tables(c), c->n, c->cars, c->d_zone0, seed, travel, d_counts, c->cu_count,
                                      [&](int what) { prof_begin(c, what); }, [&](int what) { prof_end(c, what); }, g_last_error, false, nullptr, side);
        rc = parked_pass(rc);
        if (rc == CPM_OK) c->last_form = c->zg.last_form;
        if (rc == CPM_OK) c->last_hour = c->zg.last_hour_counted;
        if (rc == CPM_OK) c->last_cells = c->zg.last_cells;
        if (rc == CPM_OK && c->h_status && !c->status_pending) {
            c->h_status[1] = 0;
            if (hipMemcpyAsync(c->h_status, d_counts + nwords - 1, sizeof(long long), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                hipMemcpyAsync(c->h_status + 1, c->zg.maxn, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                hipEventRecord(c->status_ev, c->stream) == hipSuccess)
                c->status_pending = true;
        }
        return rc;
    }
    {   // these kernels search the f64 CDF rows
        int32_t rc_cdf = ensure_full_cdf(c);
        if (rc_cdf != CPM_OK) return rc_cdf;
    }
    if (kernel == CPM_KERNEL_ZONE_LDS) {
        return parked_pass(cpm::exact_run(c->zx, c->stream, c->d_pdrive, c->d_cdf, static_cast<int>(c->Z), c->Zp, static_cast<int>(c->T), c->n, c->cars,
                                          c->d_zone0, seed, travel, c->d_dm, d_counts, c->cu_count, [&](int what) { prof_begin(c, what); },
                                          [&](int what) { prof_end(c, what); }, g_last_error, false, nullptr, side));
    }
    int32_t rc = ensure_rec(c);
    if (rc != CPM_OK) return rc;
    for (int t = 0; t < c->T; ++t) {
        const uint32_t *zin = (t == 0) ? c->d_zone0 : c->d_rec + static_cast<size_t>(t - 1) * c->n;
        uint32_t *out = c->d_rec + static_cast<size_t>(t) * c->n;
        prof_begin(c);
        rc = launch_step_car(c, zin, out, t, static_cast<uint32_t>(c->T - 1 + t), seed, travel, tt_sum);
        prof_end(c);
        if (rc != CPM_OK) return rc;
        if (fd.any()) {
            rc = cpm::flows_hour_from_cars(c->stream, fd, zin, nullptr, out, c->n, static_cast<int>(c->Z), t, g_last_error);
            if (rc != CPM_OK) return rc;
        }
        if (sd.any()) HIP_TRY(cpm::stays_launch_cars(c->stream, nullptr, zin, nullptr, out, c->n, static_cast<int>(c->Z), static_cast<int>(c->T), t, sd));
        if (cd.any()) HIP_TRY(cpm::charge_launch_cars(c->stream, nullptr, zin, nullptr, out, c->n, static_cast<int>(c->Z), static_cast<int>(c->T), t, c->cars, seed, cd));
    }
    // the per-car record of the day (cpm_paths.h): d_rec is that record, hour by hour in car order
    if (pd.any()) HIP_TRY(hipMemcpyAsync(pd.paths, c->d_rec, sizeof(uint32_t) * static_cast<size_t>(c->T) * c->n, hipMemcpyDeviceToDevice, c->stream));
    return parked_pass(launch_histogram(c, d_counts));
}

// the IVP on a layout that cannot overflow: exact buckets when the row fits LDS, one thread per car otherwise
int32_t ivp_exact(cpm_ctx *c, uint64_t seed)
{
    {
        int32_t rc_cdf = ensure_full_cdf(c);
        if (rc_cdf != CPM_OK) return rc_cdf;
    }
    const bool exact = pick_kernel(c) != CPM_KERNEL_CAR && cpm::exact_path_fits(static_cast<int>(c->Z));
    c->last_kernel = exact ? CPM_KERNEL_ZONE_LDS : CPM_KERNEL_CAR;
    c->last_batch_fleets = 0;
    c->last_hour = 0;
    c->last_cells = cpm::LaunchCells{};
    c->last_form = -1;
    if (exact) {
        return cpm::exact_run(c->zx, c->stream, c->d_pdrive, c->d_cdf, static_cast<int>(c->Z), c->Zp, static_cast<int>(c->T), c->n, c->cars,
                              c->d_zone0, seed, false, nullptr, c->d_counts, c->cu_count, [](int) {}, [](int) {}, g_last_error, true, c->d_zone0);
    }
    // src/solveinitialvalueproblem.jl:8 : t = 1:(T-1), state update unconditional (:53)
    for (int t = 0; t < c->T - 1; ++t) {
        int32_t rc = launch_step_car(c, c->d_zone0, c->d_ztmp, t, static_cast<uint32_t>(t), seed, false, nullptr);
        if (rc != CPM_OK) return rc;
        c->d_zone0.swap(c->d_ztmp);  // flag bit is masked off by every reader
    }
    return CPM_OK;
}

// The IVP on the grouped layout: new state beside the old one (d_ztmp), status word copied to pinned memory behind it.
int32_t ivp_grouped(cpm_ctx *c, uint64_t seed)
{
    c->zx.buckets0_valid = false;  // the current state's grouped buckets may be cached (zg); everything else is stale once the IVP is committed
    c->zb.buckets0_valid = false;
    int32_t rc = ensure_narrow(c);
    if (rc != CPM_OK) return rc;
    rc = cpm::grouped_run(c->zg, c->stream, grouped_tables(c), c->n, c->cars, c->d_zone0, seed, false, c->d_counts, c->cu_count,
                                  [](int) {}, [](int) {}, g_last_error, true, c->d_ztmp);
    if (rc != CPM_OK) return rc;
    c->ivp_form = c->zg.last_form;
    c->ivp_cells = c->zg.last_cells;
    c->h_ivp_status[1] = 0;
    HIP_TRY(hipMemcpyAsync(c->h_ivp_status, c->d_counts + 2 * c->T * c->Z + 1, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_ivp_status + 1, c->zg.maxn, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return CPM_OK;
}

// Commit (or repeat) an IVP that was enqueued on the grouped layout.  Called before anything reads or replaces the car
// state or the tables.  Blocks until the IVP has drained.
int32_t finish_ivp(cpm_ctx *c)
{
    if (!c->ivp_pending) return CPM_OK;
    c->ivp_pending = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->zg.set_parts(static_cast<uint32_t>(c->h_ivp_status[1]), static_cast<uint32_t>(c->h_ivp_status[1] >> 32));
    auto commit = [&]() -> int32_t {
        c->d_zone0.swap(c->d_ztmp);
        c->last_kernel = CPM_KERNEL_ZONE_GROUPED;
        c->last_form = c->ivp_form;
        c->last_batch_fleets = 0;
        c->last_hour = 0;
        c->last_cells = c->ivp_cells;
        HIP_TRY(cpm::grouped_commit_ivp(c->zg, c->stream));
        return CPM_OK;
    };
    if (c->h_ivp_status[0] == 0) return commit();
    // A bucket or a run outgrew its region (or a block of a one-launch form gave up waiting): d_zone0 is untouched.  Run the IVP
    // again with twice the regions while the problem still fits (two launches per hour after a bail-out), else on the exact layout
    // (and stay there).  Every discarded attempt counts as a repeat.
    while (pick_kernel(c) == CPM_KERNEL_ZONE_GROUPED && absorb_status(c, c->h_ivp_status[0])) {
        ++c->steps_repeated;
        int32_t rc = ivp_grouped(c, c->ivp_seed);
        if (rc != CPM_OK) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->zg.set_parts(static_cast<uint32_t>(c->h_ivp_status[1]), static_cast<uint32_t>(c->h_ivp_status[1] >> 32));
        if (c->h_ivp_status[0] == 0) return commit();
    }
    ++c->steps_repeated;
    if (c->kernel == CPM_KERNEL_AUTO) c->grouped_overflowed = true;
    c->zx.buckets0_valid = false;
    c->zg.buckets0_valid = false;
    c->zb.buckets0_valid = false;
    return ivp_exact(c, c->ivp_seed);
}

int32_t ivp_enqueue(cpm_ctx *c, uint64_t seed)
{
    if (!c->have_pdrive || !c->have_cdf) return fail(CPM_ERR_STATE, "solve_ivp: p_drive / p_dest not set");
    if (!c->have_state) return fail(CPM_ERR_STATE, "solve_ivp: no car state");
    int32_t rc = finish_ivp(c);
    if (rc != CPM_OK) return rc;
    if (c->n == 0) {  // (nothing to run: the record names the family all the same)
        c->last_kernel = pick_kernel(c);
        c->last_form = c->last_kernel == CPM_KERNEL_ZONE_GROUPED ? 0 : -1;
        c->last_batch_fleets = 0;
        c->last_hour = 0;
        c->last_cells = cpm::LaunchCells{};
        return CPM_OK;
    }
    if (pick_kernel(c) == CPM_KERNEL_ZONE_GROUPED && grouped_fits(c, c->zg.cap_mult)) {
        rc = ivp_grouped(c, seed);
        if (rc != CPM_OK) return rc;
        c->ivp_pending = true;
        c->ivp_seed = seed;
        return CPM_OK;
    }
    c->zx.buckets0_valid = false;
    c->zg.buckets0_valid = false;
    c->zb.buckets0_valid = false;
    return ivp_exact(c, seed);
}

// The blocking resample: the count tensor of a valid step in c->h_counts (c->d_counts, status word included).  Leaves c->kernel
// changed when it had to fall back to a layout that cannot overflow: the caller restores it.
int32_t resample_blocking(cpm_ctx *c, uint64_t seed, uint32_t flags, cpm::SideDest side = cpm::SideDest{})
{
    int32_t rc = resample_enqueue(c, seed, flags, c->d_counts, side);
    const size_t zt = static_cast<size_t>(c->Z * c->T), nwords = 2 * zt + 2;
    auto fetch = [&]() -> int32_t {  // the count tensor, Σ time and the status word: one copy into pinned memory, one wait
        HIP_TRY(hipMemcpyAsync(c->h_counts, c->d_counts, sizeof(int64_t) * nwords, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->status_pending) c->zg.set_parts(static_cast<uint32_t>(c->h_status[1]), static_cast<uint32_t>(c->h_status[1] >> 32));  // (how the next grouped step is launched)
        c->status_pending = false;  // this step's status word is dealt with here: resample_enqueue must not grow the regions for it again
        return CPM_OK;
    };
    if (rc == CPM_OK) rc = fetch();
    // a bucket or a run outgrew its region (or a block of a one-launch form gave up waiting): again with twice the regions while the
    // problem still fits (two launches per hour after a bail-out) ...  (each discarded attempt: CPM_INFO_STEPS_REPEATED)
    while (rc == CPM_OK && c->h_counts[nwords - 1] != 0 && pick_kernel(c) == CPM_KERNEL_ZONE_GROUPED && absorb_status(c, c->h_counts[nwords - 1])) {
        ++c->steps_repeated;
        rc = resample_enqueue(c, seed, flags, c->d_counts, side);
        if (rc == CPM_OK) rc = fetch();
    }
    if (rc == CPM_OK && c->h_counts[nwords - 1] != 0) {  // ... else on a layout that cannot overflow
        ++c->steps_repeated;
        if (pick_kernel(c) == CPM_KERNEL_ZONE_GROUPED) c->grouped_overflowed = true;
        c->kernel = cpm::exact_path_fits(static_cast<int>(c->Z)) ? CPM_KERNEL_ZONE_LDS : CPM_KERNEL_CAR;
        rc = resample_enqueue(c, seed, flags, c->d_counts, side);
        if (rc == CPM_OK) rc = fetch();
    }
    return rc;
}

// The kernel choice is overridden for one blocking call only, whichever way the call ends: by the call itself (cpm_resample's compat
// route takes the per-car kernel) or by resample_blocking's fallback to a layout that cannot overflow.
struct KernelGuard {
    cpm_ctx *c;
    int saved;
    explicit KernelGuard(cpm_ctx *c_) : c(c_), saved(c_->kernel) {}
    KernelGuard(const KernelGuard &) = delete;
    ~KernelGuard() { c->kernel = saved; }
};

// What every blocking resample call does between its argument checks and its own buffers: the guard, then the pending IVP -- committed
// with the caller's kernel choice, not with an override the call applies behind this.  rc: finish_ivp's.
struct BlockingCall {
    KernelGuard guard;
    int32_t rc;
    explicit BlockingCall(cpm_ctx *c) : guard(c), rc(finish_ivp(c)) {}
};

// fleet b's count tensor from h (c->h_counts unless the batch call names a block of its own) into the caller's arrays
void copy_counts(const cpm_ctx *c, int64_t *parking, int64_t *driving, int64_t *sum_tt_q16, int b = 0, const int64_t *h = nullptr)
{
    if (!h) h = c->h_counts;
    const size_t zt = static_cast<size_t>(c->Z * c->T);
    std::memcpy(parking + b * zt, h, sizeof(int64_t) * zt);
    std::memcpy(driving + b * zt, h + zt, sizeof(int64_t) * zt);
    if (sum_tt_q16) sum_tt_q16[b] = h[2 * zt];
}

// mean_sum of createpdrive (src/createpdrive.jl:10-21), once per datamatrix / distance matrix: from the dataset's compact rows, or the
// Z x Z x T pass over the datamatrix
int32_t ensure_pdrive_mean(cpm_ctx *c)
{
    HIP_TRY(c->d_pdrive_mean.reserve(static_cast<size_t>(c->Z * c->T)));
    if (c->pdrive_mean_valid) return CPM_OK;
    int32_t rc_ds = ensure_dataset(c);
    if (rc_ds != CPM_OK) return rc_ds;
    if (c->ds_ok) {
        hipLaunchKernelGGL(cpm::k_ds_pdrive, dim3(cpm::ds_grid(c->T * c->Z)), dim3(cpm::kDsThreads * cpm::kDsRows), 0, c->stream, c->d_ds_cells, c->d_ds_cnt,
                           cpm::kDsCap, c->T * c->Z, static_cast<int>(c->Z), c->d_dist, c->d_pdrive_mean);
    } else {
        dim3 grid(nblk(c->Z, 64), static_cast<unsigned>(c->T));
        hipLaunchKernelGGL(cpm::k_pdrive_mean, grid, dim3(64), 0, c->stream, c->d_dm, c->d_dist, c->d_pdrive_mean, static_cast<int>(c->Z));
    }
    HIP_TRY(hipGetLastError());
    c->pdrive_mean_valid = true;
    return CPM_OK;
}

// ------------------------------------------------------------------ batch (include/cpm_batch.h)
int32_t ensure_batch_tables(cpm_ctx *c, int B)
{
    const size_t cells = static_cast<size_t>(B) * c->T * c->Z;
    if (c->d_pdrive_b.fits(cells) && c->d_thr_b.fits(cells)) return CPM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the tables in use by steps in flight are replaced)
    c->batch_B = 0;
    HIP_TRY(c->d_pdrive_b.reserve(cells));
    HIP_TRY(c->d_thr_b.reserve(cells));
    return CPM_OK;
}

// A fleet's table in place of the context's own p_drive for the single-fleet step; the context's table, its flag and its kernel
// choice are back when the object goes, on every path.
struct FleetTable {
    cpm_ctx *c;
    double *pdrive;
    long long *thr;
    bool have;
    int kernel;
    explicit FleetTable(cpm_ctx *c_) : c(c_), pdrive(c_->d_pdrive), thr(c_->d_thr), have(c_->have_pdrive), kernel(c_->kernel) {}
    void use(int b)
    {
        const size_t off = static_cast<size_t>(b) * c->T * c->Z;
        c->d_pdrive = c->d_pdrive_b + off;
        c->d_thr = c->d_thr_b + off;
        c->have_pdrive = true;
        c->kernel = kernel;
    }
    ~FleetTable()
    {
        c->d_pdrive = pdrive;
        c->d_thr = thr;
        c->have_pdrive = have;
        c->kernel = kernel;
    }
};

int32_t batch_ready(cpm_ctx *c, const uint64_t *seeds, uint32_t flags)
{
    if (!seeds) return fail(CPM_ERR_ARG, "resample_batch: null seeds");
    if (c->batch_B < 1) return fail(CPM_ERR_STATE, "resample_batch: no batch tables (cpm_set_p_drive_batch / cpm_build_p_drive_batch)");
    if (!c->have_cdf) return fail(CPM_ERR_STATE, "resample_batch: p_dest not set");
    if (!c->have_state) return fail(CPM_ERR_STATE, "resample_batch: no car state (cpm_init_states / cpm_set_state)");
    if ((flags & CPM_FLAG_TRAVEL) && !c->have_dm()) return fail(CPM_ERR_STATE, "CPM_FLAG_TRAVEL needs cpm_set_datamatrix");
    return finish_ivp(c);
}

// After an overflow of the batch's regions: twice the regions while the problem still fits (grow_grouped's rule, for the batch's own
// cap_mult); the next run re-buckets the state.  false: no room to grow.
bool grow_batch(cpm_ctx *c)
{
    const int next = c->zb.cap_mult * 2;
    if (next > cpm::kMaxCapMult || !cpm::grouped_path_fits(c->n, static_cast<int>(c->Z), next)) return false;
    c->zb.cap_mult = next;
    c->zb.buckets0_valid = false;
    return true;
}

// what the last asynchronous batch step's status words ask of the batch, once that step has drained (no wait): a bucket or a run of a
// fleet outgrew its region -> twice the regions for the steps that follow (that step's fleets are the caller's to repeat)
void absorb_batch_status(cpm_ctx *c)
{
    if (!c->bstatus_pending || hipEventQuery(c->bstatus_ev) != hipSuccess) return;
    c->bstatus_pending = false;
    if (*c->h_bstatus != 0) (void)grow_batch(c);
}

// the batched kernels run when the single path would take the grouped family for this problem (asked with a fleet's table in place)
// and the batch's own regions fit
bool batch_grouped(const cpm_ctx *c)
{
    return c->n > 0 && pick_kernel(c) == CPM_KERNEL_ZONE_GROUPED && grouped_fits(c, c->zg.cap_mult) && cpm::grouped_path_fits(c->n, static_cast<int>(c->Z), c->zb.cap_mult);
}

// fleets k of `tabs` (their tables, seeds, count tensors d_counts + outs[k] * nwords) on the batched kernels, in sub-batches
int32_t batch_enqueue(cpm_ctx *c, const std::vector<uint64_t> &seeds, const std::vector<int32_t> &tabs, const std::vector<int32_t> &outs, uint32_t flags,
                      int64_t *d_counts)
{
    const bool travel = (flags & CPM_FLAG_TRAVEL) != 0;
    if (travel) {
        int32_t rc_tt = ensure_travel_tables(c);
        if (rc_tt != CPM_OK) return rc_tt;
    }
    const int nfl = static_cast<int>(tabs.size());
    const int sub = cpm::BatchWork::sub_batch(c->n, static_cast<int>(c->Z), static_cast<int>(c->T), c->zb.cap_mult, nfl);
    const cpm::GroupedTables tb = grouped_tables(c);
    for (int k0 = 0; k0 < nfl; k0 += sub) {
        const int nf = std::min(sub, nfl - k0);
        int32_t rc = cpm::batch_run(c->zb, c->stream, tb, c->n, c->cars, c->d_zone0, c->d_thr_b, seeds.data() + k0, tabs.data() + k0, outs.data() + k0, nf,
                                    travel, d_counts, c->cu_count, g_last_error);
        if (rc != CPM_OK) return rc;
    }
    return CPM_OK;
}

// ------------------------------------------------------------------ expected densities (include/cpm_expected.h)
int32_t exp_device_check()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(CPM_ERR_HIP, "expected: no HIP device: this library has no CPU path");
    return CPM_OK;
}

// l, r, the residual lists and the row-total check of the installed p_destin tables (cpm_expected.h): once per table.  Synchronises
// (the check is read back).
int32_t ensure_exp_aux(cpm_ctx *c)
{
    if (c->exp_aux_valid) return CPM_OK;
    c->exp_trip_valid = false;  // (the trip weights read l and r: never older than these)
    int32_t rc = ensure_dense_p(c);
    if (rc != CPM_OK) return rc;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t rows = static_cast<size_t>(Z) * T;
    HIP_TRY(c->d_exp_ell.reserve(rows));
    HIP_TRY(c->d_exp_r.reserve(rows));
    HIP_TRY(c->d_exp_start.reserve(rows + T));
    HIP_TRY(c->d_exp_list.reserve(rows));
    HIP_TRY(c->d_exp_bad.reserve(1));
    HIP_TRY(c->h_exp_bad.reserve(1));
    HIP_TRY(hipMemsetAsync(c->d_exp_bad, 0xff, sizeof(unsigned long long), c->stream));
    const dim3 grid(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T));
    cpm::launch(cpm::k_exp_aux, grid, dim3(cpm::kExpBlock), 0, c->stream, c->d_p.get(), c->d_last, Z, c->d_exp_ell.get(), c->d_exp_r.get(),
                c->d_exp_bad.get());
    HIP_TRY(hipGetLastError());
    const size_t lds = sizeof(int) * static_cast<size_t>(Z);
    HIP_TRY(cpm::lds_opt_in<cpm::k_exp_lists>(lds));
    cpm::launch(cpm::k_exp_lists, grid, dim3(cpm::kExpBlock), lds, c->stream, c->d_exp_ell.get(), Z, c->d_exp_start.get(), c->d_exp_list.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_exp_bad, c->d_exp_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const unsigned long long bad = *c->h_exp_bad;
    if (bad != ~0ull)
        return fail(CPM_ERR_TABLE, "expected: the row total of hour %llu, origin %llu exceeds 1: not the sampler's law (include/cpm_expected.h)",
                    bad / static_cast<unsigned long long>(Z) + 1, bad % static_cast<unsigned long long>(Z) + 1);
    c->exp_aux_valid = true;
    return CPM_OK;
}

int32_t exps_no_rows()
{
    return fail(CPM_ERR_STATE, "expected_sparse: the installed p_destin tables have no compact rows (cpm_build_p_dest on a sparse datamatrix, or "
                               "cpm_set_p_dest under CPM_OPT_SPARSE_UPLOAD, produce them)");
}

// The same per-table arrays from the compact rows of sparse tables, and the rows' transpose (cpm_expected_sparse.h): once per table.
// d_p is neither read nor built, and exp_aux_valid is left alone: launch_exp_hour reads d_p on the strength of ensure_exp_aux.
// Synchronises once (the row-total check and the number of cells are read back).
int32_t ensure_exps(cpm_ctx *c)
{
    if (!c->sparse_tables) return exps_no_rows();
    if (c->exps_valid) return CPM_OK;
    c->exps_trip_valid = false;  // (the sparse trip weights read l and r: never older than these)
    c->exps_dp_gen = -1;         // (the transposed tangent follows the cells' order: never older than it)
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    if (Z > cpm::kExpsMaxZ) return fail(CPM_ERR_STATE, "expected_sparse: more than %d zones", cpm::kExpsMaxZ);
    const int64_t nrows = static_cast<int64_t>(Z) * T;
    const size_t rows = static_cast<size_t>(nrows), cols = rows + T;
    HIP_TRY(c->d_exps_ell.reserve(rows));
    HIP_TRY(c->d_exps_r.reserve(rows));
    HIP_TRY(c->d_exps_start.reserve(cols));
    HIP_TRY(c->d_exps_list.reserve(rows));
    HIP_TRY(c->d_exps_colptr.reserve(cols + 1));
    HIP_TRY(c->d_exps_stat.reserve(2));
    HIP_TRY(c->h_exps_stat.reserve(2));
    HIP_TRY(c->d_exps_cur.reserve(cols));
    uint32_t *const d_cur = c->d_exps_cur;  // the columns' counts, then the fill's tickets
    HIP_TRY(hipMemsetAsync(c->d_exps_stat, 0xff, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(d_cur, 0, sizeof(uint32_t) * cols, c->stream));
    const dim3 rgrid(cpm::ds_grid(nrows)), rblock(cpm::kDsThreads * cpm::kDsRows);
    cpm::launch(cpm::k_exps_aux, rgrid, rblock, 0, c->stream, c->d_sp.get(), c->d_sj.get(), c->d_scnt.get(), cpm::kDsCap, nrows, Z, c->d_last,
                c->d_exps_ell.get(), c->d_exps_r.get(), c->d_exps_stat.get(), d_cur);
    HIP_TRY(hipGetLastError());
    const dim3 grid(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T));
    const size_t lds = sizeof(int) * static_cast<size_t>(Z);
    HIP_TRY(cpm::lds_opt_in<cpm::k_exp_lists>(lds));
    cpm::launch(cpm::k_exp_lists, grid, dim3(cpm::kExpBlock), lds, c->stream, c->d_exps_ell.get(), Z, c->d_exps_start.get(), c->d_exps_list.get());
    HIP_TRY(hipGetLastError());
    cpm::launch(cpm::k_exps_scan, dim3(1), dim3(cpm::kExpBlock), 0, c->stream, d_cur, cols, c->d_exps_colptr.get(), c->d_exps_stat.get() + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_exps_stat, c->d_exps_stat, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const unsigned long long bad = c->h_exps_stat[0];
    if (bad != ~0ull)
        return fail(CPM_ERR_TABLE, "expected: the row total of hour %llu, origin %llu exceeds 1: not the sampler's law (include/cpm_expected.h)",
                    bad / static_cast<unsigned long long>(Z) + 1, bad % static_cast<unsigned long long>(Z) + 1);
    const size_t cells = static_cast<size_t>(c->h_exps_stat[1]);
    if (cells > rows * cpm::kDsCap) return fail(CPM_ERR_HIP, "expected_sparse: %zu cells counted in rows that hold %zu", cells, rows * cpm::kDsCap);
    HIP_TRY(c->d_exps_o.reserve(cells));
    HIP_TRY(c->d_exps_p.reserve(cells));
    DevBuf<double> d_tmp;  // the columns' cells in the order the tickets came, values then origins: freed behind the sort (hipFree waits for it)
    HIP_TRY(d_tmp.reserve(cells + (cells + 1) / 2));
    double *const d_tmp_p = d_tmp;
    uint32_t *const d_tmp_o = reinterpret_cast<uint32_t *>(d_tmp_p + cells);
    HIP_TRY(hipMemsetAsync(d_cur, 0, sizeof(uint32_t) * cols, c->stream));
    cpm::launch(cpm::k_exps_fill, rgrid, rblock, 0, c->stream, c->d_sp.get(), c->d_sj.get(), c->d_scnt.get(), cpm::kDsCap, nrows, Z, c->d_exps_colptr.get(),
                d_cur, d_tmp_o, d_tmp_p);
    HIP_TRY(hipGetLastError());
    cpm::launch(cpm::k_exps_sort, dim3(static_cast<unsigned>(Z), static_cast<unsigned>(T)), dim3(cpm::kExpBlock), 0, c->stream, c->d_exps_colptr.get(),
                d_tmp_o, d_tmp_p, Z, c->d_exps_o.get(), c->d_exps_p.get());
    HIP_TRY(hipGetLastError());
    c->exps_cells = cells;
    c->exps_valid = true;
    return CPM_OK;
}

// the installed p_destin tables are there for the propagation to read (what: the family that asks, as its error text names it)
int32_t exp_tables_ready(const cpm_ctx *c, const char *what)
{
    if (!c->have_cdf || !(c->d_p || c->sparse_tables) || !c->d_last) return fail(CPM_ERR_STATE, "%s: p_dest not set", what);
    return CPM_OK;
}

template <int NB>
void launch_exp_hour(cpm_ctx *c, int t, const double *q_cur, const double *q_next, size_t q_stride, const double *pi_in, const double *x_in,
                     double *pi_out, double *x_out, double *park, double *drv, size_t out_stride, int Zs, int nf)
{
    const int Z = static_cast<int>(c->Z);
    const size_t row = static_cast<size_t>(t) * Z;
    cpm::launch(cpm::k_exp_hour<NB>, dim3(nblk(Z, cpm::kExpRows)), dim3(cpm::kExpBlock), 0, c->stream, c->d_p + row * Z, c->d_last + row, c->d_exp_r + row,
                c->d_exp_start + static_cast<size_t>(t) * (Z + 1), c->d_exp_list + row, q_cur, q_next, q_stride, pi_in, x_in, pi_out, x_out, park, drv,
                out_stride, Z, Zs, nf);
}

// the same hour from the transposed compact rows (k_exps_hour; ensure_exps built them)
template <int NB>
void launch_exps_hour(cpm_ctx *c, int t, const double *q_cur, const double *q_next, size_t q_stride, const double *pi_in, const double *x_in,
                      double *pi_out, double *x_out, double *park, double *drv, size_t out_stride, int Zs, int nf)
{
    const int Z = static_cast<int>(c->Z);
    const size_t row = static_cast<size_t>(t) * Z;
    cpm::launch(cpm::k_exps_hour<NB>, dim3(nblk(Z, cpm::kExpRows)), dim3(cpm::kExpBlock), 0, c->stream, c->d_exps_colptr + static_cast<size_t>(t) * (Z + 1),
                c->d_exps_o.get(), c->d_exps_p.get(), t & 1, c->d_last + row, c->d_exps_r + row, c->d_exps_start + static_cast<size_t>(t) * (Z + 1),
                c->d_exps_list + row, q_cur, q_next, q_stride, pi_in, x_in, pi_out, x_out, park, drv, out_stride, Z, Zs, nf);
}

// The recurrence for B fleets whose p_drive tables ([T][Z] each) lie q_stride words apart at pd: enqueued on the context's stream.
// out: [B][2][T][Z].  pi_next: [Z] or nullptr (B = 1).  sparse: the hours read the transposed compact rows (k_exps_hour) instead of d_p.
int32_t expected_enqueue(cpm_ctx *c, const double *d_pi0, uint32_t flags, int B, const double *pd, size_t q_stride, double *out, double *pi_next,
                         bool sparse = false)
{
    int32_t rc = exp_tables_ready(c, "expected");
    if (rc != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps(c) : ensure_exp_aux(c)) != CPM_OK) return rc;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const int Zs = (Z + 1) & ~1;  // (every fleet's vector starts on a 16-byte line)
    HIP_TRY(c->d_exp_ws.reserve(4 * static_cast<size_t>(B) * Zs));  // (a grow frees first: hipFree waits for what still reads the old workspace)
    const size_t half = c->d_exp_ws.cap / 4;                         // (the fleets it was last grown for, [Zs] each)
    double *ws_pi[2] = {c->d_exp_ws, c->d_exp_ws + half};
    double *ws_x[2] = {c->d_exp_ws + 2 * half, c->d_exp_ws + 3 * half};
    const size_t zt = static_cast<size_t>(Z) * T, out_stride = 2 * zt;
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0;  // operators in front of the day
    // step s applies the operator of hour (s < pre ? s : s - pre); the state behind step pre - 1 (or pi_0) is hour 0 of the outputs
    cpm::launch(cpm::k_exp_init, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(B)), dim3(cpm::kExpBlock), 0, c->stream, d_pi0, pd, q_stride, Z, Zs,
                ws_pi[0], ws_x[0], pre == 0 ? out : nullptr, pre == 0 ? out + zt : nullptr, out_stride);
    HIP_TRY(hipGetLastError());
    const int steps = pre + T;
    for (int s = 0; s < steps; ++s) {
        const int t = s < pre ? s : s - pre;
        const int day_next = s + 1 - pre;  // the hour of the day whose state this step produces (< 0: still in front of it)
        const bool more = s + 1 < steps;
        const int t_next = s + 1 < pre ? s + 1 : s + 1 - pre;
        const int in = s & 1, ot = in ^ 1;
        for (int f0 = 0; f0 < B; f0 += cpm::kExpMaxNB) {
            const int nf = std::min(B - f0, cpm::kExpMaxNB);
            const double *q_cur = pd + f0 * q_stride + static_cast<size_t>(t) * Z;
            const double *q_next = more ? pd + f0 * q_stride + static_cast<size_t>(t_next) * Z : nullptr;
            double *park = nullptr, *drv = nullptr;
            if (day_next >= 0 && day_next < T) {
                park = out + f0 * out_stride + static_cast<size_t>(day_next) * Z;
                drv = park + zt;
            } else if (day_next == T && pi_next) {
                park = pi_next;  // (B = 1)
            }
            const size_t w0 = static_cast<size_t>(f0) * Zs;
            // the smallest instantiation that holds the pass (fleets beyond nf repeat the last one and are not stored)
            using Go = void (*)(cpm_ctx *, int, const double *, const double *, size_t, const double *, const double *, double *, double *, double *, double *,
                                size_t, int, int);
            const Go go = sparse ? (nf > 4 ? Go(launch_exps_hour<8>) : nf > 2 ? Go(launch_exps_hour<4>) : nf > 1 ? Go(launch_exps_hour<2>) : Go(launch_exps_hour<1>))
                                 : (nf > 4 ? Go(launch_exp_hour<8>) : nf > 2 ? Go(launch_exp_hour<4>) : nf > 1 ? Go(launch_exp_hour<2>) : Go(launch_exp_hour<1>));
            go(c, t, q_cur, q_next, q_stride, ws_pi[in] + w0, ws_x[in] + w0, ws_pi[ot] + w0, ws_x[ot] + w0, park, drv, out_stride, Zs, nf);
        }
        HIP_TRY(hipGetLastError());
    }
    return CPM_OK;
}

int32_t exp_flags_check(uint32_t flags)
{
    if (flags & ~CPM_EXPECT_IVP) return fail(CPM_ERR_ARG, "expected: unknown flag bits 0x%x", flags);
    return CPM_OK;
}

// What every entry of the expected family begins with, in front of its own null-argument checks ...
int32_t exp_enter(const cpm_ctx *c)
{
    int32_t rc = exp_device_check();
    if (rc != CPM_OK) return rc;
    if (!c) return fail(CPM_ERR_ARG, "null context");
    return CPM_OK;
}

// ... and, behind them, what the entries that read p_drive tables go on with: the flags, the context's device and stream, and the
// tables themselves -- the context's own p_drive (B = 1) or the batch tables, Z * T words apart.
struct ExpTables {
    int B = 1;
    const double *pd = nullptr;
    size_t q_stride = 0;
};
int32_t exp_tables(cpm_ctx *c, uint32_t flags, bool batch, ExpTables &tb)
{
    int32_t rc = exp_flags_check(flags);
    if (rc != CPM_OK) return rc;
    CTX_TRY(c);
    if (batch) {
        if (c->batch_B < 1) return fail(CPM_ERR_STATE, "expected: no batch tables (cpm_set_p_drive_batch / cpm_build_p_drive_batch)");
        tb = ExpTables{c->batch_B, c->d_pdrive_b, static_cast<size_t>(c->Z * c->T)};
    } else {
        if (!c->have_pdrive) return fail(CPM_ERR_STATE, "expected: p_drive not set");
        tb = ExpTables{1, c->d_pdrive, 0};
    }
    return CPM_OK;
}

int32_t check_pi0(const cpm_ctx *c, const double *pi0)
{
    if (pi0)
        for (int64_t z = 0; z < c->Z; ++z)
            if (!std::isfinite(pi0[z]) || pi0[z] < 0.0) return fail(CPM_ERR_ARG, "expected: pi0 of zone %lld is NaN, infinite or negative", (long long)z + 1);
    return CPM_OK;
}

// the blocking calls' device arrays: outputs of B fleets; *tail: pi_next [Z], then pi_0 [Z], which end the allocation
int32_t ensure_exp_out(cpm_ctx *c, int B, double **tail)
{
    HIP_TRY(c->d_exp_out.reserve(static_cast<size_t>(B) * 2 * c->Z * c->T + 2 * c->Z));
    *tail = c->d_exp_out + (c->d_exp_out.cap - 2 * static_cast<size_t>(c->Z));
    return CPM_OK;
}

int32_t expected_blocking(cpm_ctx *c, const double *pi0, uint32_t flags, int B, const double *pd, size_t q_stride, double *parking, double *driving,
                          double *pi_next, bool sparse = false)
{
    int32_t rc = check_pi0(c, pi0);
    if (rc != CPM_OK) return rc;
    double *d_next = nullptr;
    if ((rc = ensure_exp_out(c, B, &d_next)) != CPM_OK) return rc;
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    double *d_pi0 = d_next + c->Z;
    if (pi0) HIP_TRY(hipMemcpyAsync(d_pi0, pi0, sizeof(double) * c->Z, hipMemcpyHostToDevice, c->stream));
    rc = expected_enqueue(c, pi0 ? d_pi0 : nullptr, flags, B, pd, q_stride, c->d_exp_out, pi_next ? d_next : nullptr, sparse);
    if (rc != CPM_OK) return rc;
    for (int b = 0; b < B; ++b) {
        HIP_TRY(hipMemcpyAsync(parking + b * zt, c->d_exp_out + b * 2 * zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(driving + b * zt, c->d_exp_out + b * 2 * zt + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    }
    if (pi_next) HIP_TRY(hipMemcpyAsync(pi_next, d_next, sizeof(double) * c->Z, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ expected travel (include/cpm_expected_travel.h)
// The trip weights of the installed p_destin tables, datamatrix and distance matrix in d_exp_w: once per table (enqueued on the
// context's stream; ensure_exp_aux synchronises when it rebuilds).
int32_t ensure_exp_trip(cpm_ctx *c)
{
    int32_t rc = exp_tables_ready(c, "expected travel");
    if (rc != CPM_OK) return rc;
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "expected travel: datamatrix not set (cpm_set_datamatrix, cpm_createdatamatrix_* or cpm_synth_datamatrix)");
    if (!c->have_dist) return fail(CPM_ERR_STATE, "expected travel: distance matrix not set (cpm_set_distance* or the dist of cpm_set_datamatrix)");
    if ((rc = ensure_exp_aux(c)) != CPM_OK) return rc;  // (the row-total check; clears exp_trip_valid when it rebuilds)
    if (c->exp_trip_valid) return CPM_OK;
    if ((rc = ensure_dense_p(c)) != CPM_OK) return rc;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t zt = static_cast<size_t>(Z) * T;
    const int nseg = cpm::trip_segments(Z, T), seg_len = cpm::trip_segment_len(Z, nseg);
    HIP_TRY(c->d_exp_w.reserve(2 * zt));
    HIP_TRY(c->d_exp_wpart.reserve(2 * zt * nseg));
    const dim3 grid(nblk(Z, cpm::kTripStrip), static_cast<unsigned>(T), static_cast<unsigned>(nseg));
    if (Z & 1) cpm::launch(cpm::k_exp_trip<true>, grid, dim3(cpm::kExpBlock), 0, c->stream, c->d_p.get(), c->d_dm.get(), c->d_dist.get(), Z, T, seg_len,
                           c->d_exp_wpart.get());
    else cpm::launch(cpm::k_exp_trip<false>, grid, dim3(cpm::kExpBlock), 0, c->stream, c->d_p.get(), c->d_dm.get(), c->d_dist.get(), Z, T, seg_len,
                           c->d_exp_wpart.get());
    HIP_TRY(hipGetLastError());
    cpm::launch(cpm::k_exp_trip_finish, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T)), dim3(cpm::kExpBlock), 0, c->stream, c->d_exp_wpart.get(),
                nseg, c->d_dm.get(), c->d_dist.get(), c->d_last, c->d_exp_ell.get(), c->d_exp_r.get(), Z, T, c->d_exp_w.get());
    HIP_TRY(hipGetLastError());
    c->exp_trip_valid = true;
    ++c->exp_trip_builds;
    return CPM_OK;
}

// The same weights from the compact rows in d_exps_w (cpm_expected_sparse_grad.h): d_p is neither read nor built, and neither
// d_exp_w nor exp_trip_builds moves.  d_exp_wpart is scratch of either build: nothing reads it afterwards.
int32_t ensure_exps_trip(cpm_ctx *c)
{
    int32_t rc = exp_tables_ready(c, "expected travel");
    if (rc != CPM_OK) return rc;
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "expected travel: datamatrix not set (cpm_set_datamatrix, cpm_createdatamatrix_* or cpm_synth_datamatrix)");
    if (!c->have_dist) return fail(CPM_ERR_STATE, "expected travel: distance matrix not set (cpm_set_distance* or the dist of cpm_set_datamatrix)");
    if ((rc = ensure_exps(c)) != CPM_OK) return rc;  // (the row-total check; clears exps_trip_valid when it rebuilds)
    if (c->exps_trip_valid) return CPM_OK;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t zt = static_cast<size_t>(Z) * T;
    const int nseg = cpm::trip_segments(Z, T), seg_len = cpm::trip_segment_len(Z, nseg);
    HIP_TRY(c->d_exps_w.reserve(2 * zt));
    HIP_TRY(c->d_exp_wpart.reserve(2 * zt * nseg));
    cpm::launch(cpm::k_exps_trip, dim3(static_cast<unsigned>(Z), static_cast<unsigned>(T)), dim3(cpm::kExpsGradBlock), 0, c->stream, c->d_sp.get(),
                c->d_sj.get(), c->d_scnt.get(), cpm::kDsCap, c->d_dm.get(), c->d_dist.get(), Z, T, seg_len, nseg, c->d_exp_wpart.get());
    HIP_TRY(hipGetLastError());
    cpm::launch(cpm::k_exp_trip_finish, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T)), dim3(cpm::kExpBlock), 0, c->stream, c->d_exp_wpart.get(),
                nseg, c->d_dm.get(), c->d_dist.get(), c->d_last, c->d_exps_ell.get(), c->d_exps_r.get(), Z, T, c->d_exps_w.get());
    HIP_TRY(hipGetLastError());
    c->exps_trip_valid = true;
    ++c->exps_trip_builds;
    return CPM_OK;
}

// seconds | km and the totals of B fleets from their expected tensors (enqueued); either output may be nullptr.  sparse: the weights
// come from the compact rows (ensure_exps_trip).
int32_t expected_travel_enqueue(cpm_ctx *c, const double *d_expected, int B, double *d_travel, double *d_totals, bool sparse = false)
{
    int32_t rc = sparse ? ensure_exps_trip(c) : ensure_exp_trip(c);
    if (rc != CPM_OK) return rc;
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    const int nchunk = static_cast<int>(nblk(static_cast<int64_t>(zt), cpm::kTravelChunk));
    if (d_totals) HIP_TRY(c->d_exp_tpart.reserve(2 * static_cast<size_t>(B) * nchunk));  // (a grow frees first: hipFree waits for its readers)
    cpm::launch(cpm::k_exp_travel, dim3(static_cast<unsigned>(nchunk), static_cast<unsigned>(B)), dim3(cpm::kExpBlock), 0, c->stream, d_expected,
                sparse ? c->d_exps_w.get() : c->d_exp_w.get(), zt, d_travel, d_totals ? c->d_exp_tpart.get() : nullptr);
    HIP_TRY(hipGetLastError());
    if (d_totals) {
        cpm::launch(cpm::k_exp_travel_total, dim3(static_cast<unsigned>(B)), dim3(64), 0, c->stream, c->d_exp_tpart.get(), nchunk, d_totals);
        HIP_TRY(hipGetLastError());
    }
    return CPM_OK;
}

// the blocking calls: the propagation into d_exp_out, the product into d_exp_trav, then the copies
int32_t expected_travel_blocking(cpm_ctx *c, const double *pi0, uint32_t flags, int B, const double *pd, size_t q_stride, double *seconds, double *km,
                                 double *totals, bool sparse = false)
{
    int32_t rc = check_pi0(c, pi0);
    if (rc != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps_trip(c) : ensure_exp_trip(c)) != CPM_OK) return rc;  // (first: a missing datamatrix is reported before any work is enqueued)
    double *d_next = nullptr;
    if ((rc = ensure_exp_out(c, B, &d_next)) != CPM_OK) return rc;
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    HIP_TRY(c->d_exp_trav.reserve(static_cast<size_t>(B) * (2 * zt + 2)));
    double *d_pi0 = d_next + c->Z;
    double *d_tot = c->d_exp_trav + c->d_exp_trav.cap / (2 * zt + 2) * 2 * zt;  // (behind the tensors of the fleets it was last grown for)
    if (pi0) HIP_TRY(hipMemcpyAsync(d_pi0, pi0, sizeof(double) * c->Z, hipMemcpyHostToDevice, c->stream));
    rc = expected_enqueue(c, pi0 ? d_pi0 : nullptr, flags, B, pd, q_stride, c->d_exp_out, nullptr, sparse);
    if (rc != CPM_OK) return rc;
    rc = expected_travel_enqueue(c, c->d_exp_out, B, c->d_exp_trav, d_tot, sparse);
    if (rc != CPM_OK) return rc;
    for (int b = 0; b < B; ++b) {
        HIP_TRY(hipMemcpyAsync(seconds + b * zt, c->d_exp_trav + b * 2 * zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(km + b * zt, c->d_exp_trav + b * 2 * zt + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    }
    if (totals) HIP_TRY(hipMemcpyAsync(totals, d_tot, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ adjoint of the expected densities (include/cpm_expected_grad.h)
// one backward product of the hour whose first row is `row`, from the compact rows (k_exps_grad_u; ensure_exps has run)
void launch_exps_grad_u(cpm_ctx *c, size_t row, const double *mu, int Zs, int nseg, int seg_len, double *part)
{
    const int Z = static_cast<int>(c->Z);
    cpm::launch(cpm::k_exps_grad_u, dim3(static_cast<unsigned>(Z)), dim3(cpm::kExpsGradBlock), 0, c->stream, c->d_sp + row * cpm::kDsCap,
                c->d_sj + row * cpm::kDsCap, c->d_scnt + row, cpm::kDsCap, mu, Z, Zs, seg_len, nseg, part);
}

// ... of a pass of nf > 1 fleets (k_exps_grad_u_b<NB>)
template <int NB>
void launch_exps_grad_u_b(cpm_ctx *c, size_t row, const double *mu, int Zs, int nseg, int seg_len, int nf, double *part)
{
    const int Z = static_cast<int>(c->Z);
    cpm::launch(cpm::k_exps_grad_u_b<NB>, dim3(static_cast<unsigned>(Z)), dim3(cpm::kExpsGradBlock), 0, c->stream, c->d_sp + row * cpm::kDsCap,
                c->d_sj + row * cpm::kDsCap, c->d_scnt + row, cpm::kDsCap, mu, Z, Zs, seg_len, nseg, nf, part);
}

// The forward propagation with the kernels of expected_enqueue (B = 1; pi_s of every operator kept, operator N - 1 not applied: nothing
// reads pi_N), then the N backward operators: enqueued on the context's stream.  cot: [2][T][Z]; gnext, grad_pi0: [Z] or nullptr;
// grad_pd: [T][Z].
// sparse: both halves read the compact rows (k_exps_hour, k_exps_grad_u) and the per-table arrays of ensure_exps.
int32_t expected_grad_enqueue(cpm_ctx *c, const double *d_pi0, uint32_t flags, const double *cot, const double *gnext, double *grad_pd, double *grad_pi0,
                              bool sparse = false)
{
    int32_t rc = exp_tables_ready(c, "expected");
    if (rc != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps(c) : ensure_exp_aux(c)) != CPM_OK) return rc;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const int Zs = (Z + 1) & ~1;  // (every vector starts on a 16-byte line)
    const int nseg = cpm::grad_segments(Z), seg_len = cpm::grad_segment_len(Z, nseg);
    const int most = 2 * T - 1;   // operators under CPM_EXPECT_IVP: the workspace is sized once
    HIP_TRY(c->d_exp_gws.reserve(static_cast<size_t>(most + 4 + nseg) * Zs));
    double *ws_pi = c->d_exp_gws;
    double *ws_x[2] = {ws_pi + static_cast<size_t>(most) * Zs, ws_pi + static_cast<size_t>(most + 1) * Zs};
    double *ws_mu[2] = {ws_pi + static_cast<size_t>(most + 2) * Zs, ws_pi + static_cast<size_t>(most + 3) * Zs};
    double *part = ws_pi + static_cast<size_t>(most + 4) * Zs;
    const double *pd = c->d_pdrive;
    const size_t zt = static_cast<size_t>(Z) * T;
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0, steps = pre + T;
    auto hour_of = [pre](int s) { return s < pre ? s : s - pre; };

    cpm::launch(cpm::k_exp_init, dim3(nblk(Z, cpm::kExpBlock), 1u), dim3(cpm::kExpBlock), 0, c->stream, d_pi0, pd, static_cast<size_t>(0), Z, Zs, ws_pi,
                ws_x[0], static_cast<double *>(nullptr), static_cast<double *>(nullptr), static_cast<size_t>(0));
    HIP_TRY(hipGetLastError());
    using Go = void (*)(cpm_ctx *, int, const double *, const double *, size_t, const double *, const double *, double *, double *, double *, double *, size_t,
                        int, int);
    const Go hour = sparse ? Go(launch_exps_hour<1>) : Go(launch_exp_hour<1>);
    for (int s = 0; s + 1 < steps; ++s) {
        const int t = hour_of(s), t_next = hour_of(s + 1);
        hour(c, t, pd + static_cast<size_t>(t) * Z, pd + static_cast<size_t>(t_next) * Z, 0, ws_pi + static_cast<size_t>(s) * Zs, ws_x[s & 1],
             ws_pi + static_cast<size_t>(s + 1) * Zs, ws_x[(s + 1) & 1], nullptr, nullptr, 0, Zs, 1);
        HIP_TRY(hipGetLastError());
    }

    const int *const d_ell = sparse ? c->d_exps_ell.get() : c->d_exp_ell.get();
    const double *const d_r = sparse ? c->d_exps_r.get() : c->d_exp_r.get();
    const double *mu = gnext;  // (nullptr: zero by construction, the product of the last operator is skipped)
    for (int s = steps - 1; s >= 0; --s) {
        const int t = hour_of(s), j = s - pre;
        const size_t row = static_cast<size_t>(t) * Z;
        if (mu) {
            const dim3 grid(nblk(Z, cpm::kGradStrip), static_cast<unsigned>(nseg));
            if (sparse) launch_exps_grad_u(c, row, mu, Zs, nseg, seg_len, part);
            else if (Z & 1) cpm::launch(cpm::k_exp_grad_u<true>, grid, dim3(cpm::kExpBlock), 0, c->stream, c->d_p + row * Z, mu, Z, Zs, seg_len, part);
            else cpm::launch(cpm::k_exp_grad_u<false>, grid, dim3(cpm::kExpBlock), 0, c->stream, c->d_p + row * Z, mu, Z, Zs, seg_len, part);
            HIP_TRY(hipGetLastError());
        }
        double *mu_out = (s == 0 && grad_pi0) ? grad_pi0 : ws_mu[s & 1];
        const double *gp = j >= 0 ? cot + static_cast<size_t>(j) * Z : nullptr;
        const double *gd = j >= 0 ? cot + zt + static_cast<size_t>(j) * Z : nullptr;
        cpm::launch(cpm::k_exp_grad_finish, dim3(nblk(Z, cpm::kFinishBlock)), dim3(cpm::kFinishBlock), 0, c->stream, part, nseg, Zs, c->d_last + row,
                    d_ell + row, d_r + row, pd + row, ws_pi + static_cast<size_t>(s) * Zs, mu, gp, gd, Z, s < pre ? 1 : 0, mu_out, grad_pd + row);
        HIP_TRY(hipGetLastError());
        mu = mu_out;
    }
    return CPM_OK;
}

int32_t expected_grad_blocking(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                               double *grad_pd, double *grad_pi0, bool sparse = false)
{
    const size_t Z = static_cast<size_t>(c->Z), zt = Z * static_cast<size_t>(c->T);
    int32_t rc = check_pi0(c, pi0);
    if (rc != CPM_OK) return rc;
    for (size_t i = 0; i < zt; ++i)
        if (!std::isfinite(g_parking[i]) || !std::isfinite(g_driving[i]))
            return fail(CPM_ERR_ARG, "expected_grad: the cotangent of zone %lld, hour %lld is not finite", (long long)(i % Z) + 1, (long long)(i / Z) + 1);
    if (g_next)
        for (size_t z = 0; z < Z; ++z)
            if (!std::isfinite(g_next[z])) return fail(CPM_ERR_ARG, "expected_grad: g_next of zone %lld is not finite", (long long)z + 1);
    HIP_TRY(c->d_exp_gio.reserve(3 * zt + 3 * Z));
    double *d_cot = c->d_exp_gio, *d_gnext = d_cot + 2 * zt, *d_grad = d_gnext + Z, *d_gpi0 = d_grad + zt, *d_pi0 = d_gpi0 + Z;
    HIP_TRY(hipMemcpyAsync(d_cot, g_parking, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_cot + zt, g_driving, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
    if (g_next) HIP_TRY(hipMemcpyAsync(d_gnext, g_next, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    if (pi0) HIP_TRY(hipMemcpyAsync(d_pi0, pi0, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    rc = expected_grad_enqueue(c, pi0 ? d_pi0 : nullptr, flags, d_cot, g_next ? d_gnext : nullptr, d_grad, grad_pi0 ? d_gpi0 : nullptr, sparse);
    if (rc != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(grad_pd, d_grad, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    if (grad_pi0) HIP_TRY(hipMemcpyAsync(grad_pi0, d_gpi0, sizeof(double) * Z, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ the adjoint along a tangent of p_destin (include/cpm_expected_grad_dest.h)
int32_t tangent_ready(const cpm_ctx *c, const char *what)
{
    if (!c->tan_valid || !c->d_tan)
        return fail(CPM_ERR_STATE, "%s: no tangent of the installed p_destin tables (cpm_set_p_dest_tangent or cpm_build_p_dest_tangent)", what);
    return CPM_OK;
}

// ... on the stored cells (include/cpm_expected_sparse_dest.h)
int32_t sdp_ready(const cpm_ctx *c, const char *what)
{
    if (!c->sdp_valid || !c->d_sdp)
        return fail(CPM_ERR_STATE, "%s: no compact tangent of the installed p_destin tables (cpm_set_p_dest_tangent_sparse or cpm_build_p_dest_tangent_sparse)", what);
    return CPM_OK;
}

// one fused backward product of the hour whose first row is `row`, from the compact rows and the compact tangent (k_exps_grad_dest_u)
void launch_exps_grad_dest_u(cpm_ctx *c, size_t row, const double *mu, int Zs, int nseg, int seg_len, double *part, double *part_dp)
{
    const int Z = static_cast<int>(c->Z);
    cpm::launch(cpm::k_exps_grad_dest_u, dim3(static_cast<unsigned>(Z)), dim3(cpm::kExpsGradBlock), 0, c->stream, c->d_sp + row * cpm::kDsCap,
                c->d_sdp + row * cpm::kDsCap, c->d_sj + row * cpm::kDsCap, c->d_scnt + row, cpm::kDsCap, mu, Z, Zs, seg_len, nseg, part, part_dp);
}

// ... of a pass of nf > 1 fleets (k_exps_grad_dest_u_b<NB>)
template <int NB>
void launch_exps_grad_dest_u_b(cpm_ctx *c, size_t row, const double *mu, int Zs, int nseg, int seg_len, int nf, double *part, double *part_dp)
{
    const int Z = static_cast<int>(c->Z);
    const unsigned groups = static_cast<unsigned>((nf + cpm::kExpsDestFleets - 1) / cpm::kExpsDestFleets);  // (nf <= NB: every group lies inside mu's NB columns)
    cpm::launch(cpm::k_exps_grad_dest_u_b<NB>, dim3(static_cast<unsigned>(Z), groups), dim3(cpm::kExpsGradBlock), 0, c->stream, c->d_sp + row * cpm::kDsCap,
                c->d_sdp + row * cpm::kDsCap, c->d_sj + row * cpm::kDsCap, c->d_scnt + row, cpm::kDsCap, mu, Z, Zs, seg_len, nseg, nf, part, part_dp);
}

// expected_grad_enqueue with the fused product and the finishing kernel of cpm_expected_grad_dest.h: the same forward propagation, the
// same workspace with the segments' sums of w behind those of a.  grad_dest: [T][Z].
// sparse: both halves read the compact rows, the product the compact tangent beside them (k_exps_hour, k_exps_grad_dest_u).
int32_t expected_grad_dest_enqueue(cpm_ctx *c, const double *d_pi0, uint32_t flags, const double *cot, const double *gnext, double *grad_pd, double *grad_pi0,
                                   double *grad_dest, bool sparse = false)
{
    int32_t rc = exp_tables_ready(c, "expected");
    if (rc != CPM_OK) return rc;
    if ((rc = sparse ? sdp_ready(c, "expected_sparse_grad_dest") : tangent_ready(c, "expected_grad_dest")) != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps(c) : ensure_exp_aux(c)) != CPM_OK) return rc;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const int Zs = (Z + 1) & ~1;  // (every vector starts on a 16-byte line)
    const int nseg = cpm::grad_segments(Z), seg_len = cpm::grad_segment_len(Z, nseg);
    const int most = 2 * T - 1;   // operators under CPM_EXPECT_IVP: the workspace is sized once
    HIP_TRY(c->d_exp_gws.reserve(static_cast<size_t>(most + 4 + 2 * nseg) * Zs));
    double *ws_pi = c->d_exp_gws;
    double *ws_x[2] = {ws_pi + static_cast<size_t>(most) * Zs, ws_pi + static_cast<size_t>(most + 1) * Zs};
    double *ws_mu[2] = {ws_pi + static_cast<size_t>(most + 2) * Zs, ws_pi + static_cast<size_t>(most + 3) * Zs};
    double *part = ws_pi + static_cast<size_t>(most + 4) * Zs;
    double *part_dp = part + static_cast<size_t>(nseg) * Zs;
    const double *pd = c->d_pdrive;
    const size_t zt = static_cast<size_t>(Z) * T;
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0, steps = pre + T;
    auto hour_of = [pre](int s) { return s < pre ? s : s - pre; };

    cpm::launch(cpm::k_exp_init, dim3(nblk(Z, cpm::kExpBlock), 1u), dim3(cpm::kExpBlock), 0, c->stream, d_pi0, pd, static_cast<size_t>(0), Z, Zs, ws_pi,
                ws_x[0], static_cast<double *>(nullptr), static_cast<double *>(nullptr), static_cast<size_t>(0));
    HIP_TRY(hipGetLastError());
    for (int s = 0; s + 1 < steps; ++s) {
        const int t = hour_of(s), t_next = hour_of(s + 1);
        (sparse ? launch_exps_hour<1> : launch_exp_hour<1>)(c, t, pd + static_cast<size_t>(t) * Z, pd + static_cast<size_t>(t_next) * Z, 0,
                                                            ws_pi + static_cast<size_t>(s) * Zs, ws_x[s & 1], ws_pi + static_cast<size_t>(s + 1) * Zs,
                                                            ws_x[(s + 1) & 1], nullptr, nullptr, 0, Zs, 1);
        HIP_TRY(hipGetLastError());
    }

    const int *const d_ell = sparse ? c->d_exps_ell.get() : c->d_exp_ell.get();
    const double *const d_r = sparse ? c->d_exps_r.get() : c->d_exp_r.get();
    const double *mu = gnext;  // (nullptr: zero by construction, the products of the last operator are skipped)
    for (int s = steps - 1; s >= 0; --s) {
        const int t = hour_of(s), j = s - pre;
        const size_t row = static_cast<size_t>(t) * Z;
        if (mu) {
            const dim3 grid(nblk(Z, cpm::kGradStrip), static_cast<unsigned>(nseg));
            if (sparse) launch_exps_grad_dest_u(c, row, mu, Zs, nseg, seg_len, part, part_dp);
            else if (Z & 1) cpm::launch(cpm::k_exp_grad_dest_u<true>, grid, dim3(cpm::kExpBlock), 0, c->stream, c->d_p + row * Z, c->d_tan + row * Z, mu, Z, Zs, seg_len,
                                   part, part_dp);
            else cpm::launch(cpm::k_exp_grad_dest_u<false>, grid, dim3(cpm::kExpBlock), 0, c->stream, c->d_p + row * Z, c->d_tan + row * Z, mu, Z, Zs, seg_len,
                             part, part_dp);
            HIP_TRY(hipGetLastError());
        }
        double *mu_out = (s == 0 && grad_pi0) ? grad_pi0 : ws_mu[s & 1];
        const double *gp = j >= 0 ? cot + static_cast<size_t>(j) * Z : nullptr;
        const double *gd = j >= 0 ? cot + zt + static_cast<size_t>(j) * Z : nullptr;
        cpm::launch(cpm::k_exp_grad_dest_finish, dim3(nblk(Z, cpm::kFinishBlock)), dim3(cpm::kFinishBlock), 0, c->stream, part, part_dp, nseg, Zs,
                    c->d_last + row, d_ell + row, d_r + row, pd + row, ws_pi + static_cast<size_t>(s) * Zs, mu, gp, gd, Z, s < pre ? 1 : 0, mu_out,
                    grad_pd + row, grad_dest + row);
        HIP_TRY(hipGetLastError());
        mu = mu_out;
    }
    return CPM_OK;
}

int32_t expected_grad_dest_blocking(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                                    double *grad_pd, double *grad_pi0, double *grad_dest, bool sparse = false)
{
    const size_t Z = static_cast<size_t>(c->Z), zt = Z * static_cast<size_t>(c->T);
    int32_t rc = check_pi0(c, pi0);
    if (rc != CPM_OK) return rc;
    for (size_t i = 0; i < zt; ++i)
        if (!std::isfinite(g_parking[i]) || !std::isfinite(g_driving[i]))
            return fail(CPM_ERR_ARG, "expected_grad_dest: the cotangent of zone %lld, hour %lld is not finite", (long long)(i % Z) + 1, (long long)(i / Z) + 1);
    if (g_next)
        for (size_t z = 0; z < Z; ++z)
            if (!std::isfinite(g_next[z])) return fail(CPM_ERR_ARG, "expected_grad_dest: g_next of zone %lld is not finite", (long long)z + 1);
    HIP_TRY(c->d_exp_gio.reserve(3 * zt + 3 * Z));
    HIP_TRY(c->d_exp_gdio.reserve(zt));
    double *d_cot = c->d_exp_gio, *d_gnext = d_cot + 2 * zt, *d_grad = d_gnext + Z, *d_gpi0 = d_grad + zt, *d_pi0 = d_gpi0 + Z;
    HIP_TRY(hipMemcpyAsync(d_cot, g_parking, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_cot + zt, g_driving, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
    if (g_next) HIP_TRY(hipMemcpyAsync(d_gnext, g_next, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    if (pi0) HIP_TRY(hipMemcpyAsync(d_pi0, pi0, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    rc = expected_grad_dest_enqueue(c, pi0 ? d_pi0 : nullptr, flags, d_cot, g_next ? d_gnext : nullptr, d_grad, grad_pi0 ? d_gpi0 : nullptr, c->d_exp_gdio, sparse);
    if (rc != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(grad_pd, d_grad, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    if (grad_pi0) HIP_TRY(hipMemcpyAsync(grad_pi0, d_gpi0, sizeof(double) * Z, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(grad_dest, c->d_exp_gdio, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ the adjoint for the fleets of a batch (include/cpm_expected_grad_batch.h)
// One backward product of a pass of nf > 1 fleets: the smallest instantiation that holds the pass.  dp_t: nullptr without the tangent.
template <int NB>
void launch_grad_u_b(cpm_ctx *c, const double *p_t, const double *dp_t, const double *mu, int Zs, int nseg, int seg_len, int nf, double *part, double *part_dp)
{
    const int Z = static_cast<int>(c->Z);
    const dim3 grid(nblk(Z, cpm::kGradStrip), static_cast<unsigned>(nseg)), block(cpm::kExpBlock);
    if (dp_t) {
        if (Z & 1) cpm::launch(cpm::k_exp_grad_dest_u_b<NB, true>, grid, block, 0, c->stream, p_t, dp_t, mu, Z, Zs, seg_len, nf, part, part_dp);
        else cpm::launch(cpm::k_exp_grad_dest_u_b<NB, false>, grid, block, 0, c->stream, p_t, dp_t, mu, Z, Zs, seg_len, nf, part, part_dp);
    } else {
        if (Z & 1) cpm::launch(cpm::k_exp_grad_u_b<NB, true>, grid, block, 0, c->stream, p_t, mu, Z, Zs, seg_len, nf, part);
        else cpm::launch(cpm::k_exp_grad_u_b<NB, false>, grid, block, 0, c->stream, p_t, mu, Z, Zs, seg_len, nf, part);
    }
}

// expected_grad_enqueue / expected_grad_dest_enqueue for B fleets whose p_drive tables lie q_stride words apart at pd.  The forward
// propagation is expected_enqueue's with pi_s of every operator and fleet kept; backward, operator-major with the passes of at most
// kExpMaxNB fleets inside an operator.  cot: [B][2][T][Z]; gnext, grad_pi0: [B][Z] or nullptr; grad_pd, grad_dest: [B][T][Z];
// grad_dest == nullptr: no tangent.  A pass of one fleet runs the B = 1 kernels.
// d_exp_gws, in vectors of Zs words: pi [2T - 1][B], x ping and pong [B] each, mu ping and pong [B8] each (B8 = B rounded up to
// whole passes; a pass's mu is [Zs][NB] at its first fleet's place), the segments' sums of one pass [nseg][kExpMaxNB], those of w
// likewise.
// where the batched adjoint keeps what its two halves share: the workspace's vectors and the geometry of the segments
struct GradBatchPlan {
    bool sparse = false;  // both halves read the compact rows and the per-table arrays of ensure_exps (the tangent, if any, is the compact one)
    int Zs = 0, nseg = 0, seg_len = 0;
    size_t nb = 0;
    double *ws_pi = nullptr, *ws_x[2] = {nullptr, nullptr}, *ws_mu[2] = {nullptr, nullptr}, *part = nullptr, *part_dp = nullptr;
};

// the checks that can refuse and the workspace of B fleets (with_dest: the call runs along the tangent)
int32_t grad_batch_plan(cpm_ctx *c, int B, bool with_dest, GradBatchPlan &pl, bool sparse = false)
{
    int32_t rc = exp_tables_ready(c, "expected");
    if (rc != CPM_OK) return rc;
    if (with_dest && (rc = sparse ? sdp_ready(c, "expected_sparse_grad_dest_batch") : tangent_ready(c, "expected_grad_dest_batch")) != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps(c) : ensure_exp_aux(c)) != CPM_OK) return rc;
    pl.sparse = sparse;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const int Zs = (Z + 1) & ~1;  // (every vector starts on a 16-byte line)
    const int nseg = cpm::grad_segments(Z), seg_len = cpm::grad_segment_len(Z, nseg);
    const int most = 2 * T - 1;   // operators under CPM_EXPECT_IVP: the workspace is sized once per B
    const size_t nb = static_cast<size_t>(B), b8 = (nb + cpm::kExpMaxNB - 1) / cpm::kExpMaxNB * cpm::kExpMaxNB;
    const size_t part_words = static_cast<size_t>(nseg) * cpm::kExpMaxNB * Zs;
    HIP_TRY(c->d_exp_gws.reserve((most * nb + 2 * nb + 2 * b8) * Zs + 2 * part_words));
    double *ws_pi = c->d_exp_gws;
    pl.Zs = Zs, pl.nseg = nseg, pl.seg_len = seg_len, pl.nb = nb;
    pl.ws_pi = ws_pi;
    pl.ws_x[0] = ws_pi + most * nb * Zs, pl.ws_x[1] = ws_pi + (most + 1) * nb * Zs;
    pl.ws_mu[0] = ws_pi + (most + 2) * nb * Zs, pl.ws_mu[1] = ws_pi + ((most + 2) * nb + b8) * Zs;
    pl.part = ws_pi + ((most + 2) * nb + 2 * b8) * Zs;
    pl.part_dp = pl.part + part_words;
    return CPM_OK;
}

// the forward half: expected_enqueue's kernels with pi_s of every operator and fleet kept (operator N - 1 is not applied)
int32_t grad_batch_forward(cpm_ctx *c, const GradBatchPlan &pl, const double *d_pi0, uint32_t flags, int B, const double *pd, size_t q_stride)
{
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T), Zs = pl.Zs;
    const size_t nb = pl.nb;
    double *const ws_pi = pl.ws_pi;
    double *const ws_x[2] = {pl.ws_x[0], pl.ws_x[1]};
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0, steps = pre + T;
    auto hour_of = [pre](int s) { return s < pre ? s : s - pre; };

    cpm::launch(cpm::k_exp_init, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(B)), dim3(cpm::kExpBlock), 0, c->stream, d_pi0, pd, q_stride, Z, Zs, ws_pi,
                ws_x[0], static_cast<double *>(nullptr), static_cast<double *>(nullptr), static_cast<size_t>(0));
    HIP_TRY(hipGetLastError());
    for (int s = 0; s + 1 < steps; ++s) {
        const int t = hour_of(s), t_next = hour_of(s + 1);
        for (int f0 = 0; f0 < B; f0 += cpm::kExpMaxNB) {
            const int nf = std::min(B - f0, cpm::kExpMaxNB);
            const size_t w0 = static_cast<size_t>(f0) * Zs;
            using Go = void (*)(cpm_ctx *, int, const double *, const double *, size_t, const double *, const double *, double *, double *, double *, double *,
                                size_t, int, int);
            const Go go = pl.sparse ? (nf > 4 ? Go(launch_exps_hour<8>) : nf > 2 ? Go(launch_exps_hour<4>) : nf > 1 ? Go(launch_exps_hour<2>) : Go(launch_exps_hour<1>))
                                    : (nf > 4 ? Go(launch_exp_hour<8>) : nf > 2 ? Go(launch_exp_hour<4>) : nf > 1 ? Go(launch_exp_hour<2>) : Go(launch_exp_hour<1>));
            go(c, t, pd + f0 * q_stride + static_cast<size_t>(t) * Z, pd + f0 * q_stride + static_cast<size_t>(t_next) * Z, q_stride,
               ws_pi + static_cast<size_t>(s) * nb * Zs + w0, ws_x[s & 1] + w0, ws_pi + static_cast<size_t>(s + 1) * nb * Zs + w0, ws_x[(s + 1) & 1] + w0, nullptr,
               nullptr, 0, Zs, nf);
        }
        HIP_TRY(hipGetLastError());
    }
    return CPM_OK;
}

// the backward half: operator-major with the passes of at most kExpMaxNB fleets inside an operator
int32_t grad_batch_backward(cpm_ctx *c, const GradBatchPlan &pl, uint32_t flags, int B, const double *pd, size_t q_stride, const double *cot,
                            const double *gnext, double *grad_pd, double *grad_pi0, double *grad_dest)
{
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T), Zs = pl.Zs, nseg = pl.nseg, seg_len = pl.seg_len;
    const size_t nb = pl.nb;
    double *const ws_pi = pl.ws_pi;
    double *const ws_mu[2] = {pl.ws_mu[0], pl.ws_mu[1]};
    double *const part = pl.part, *const part_dp = pl.part_dp;
    const size_t zt = static_cast<size_t>(Z) * T, cot_stride = 2 * zt;
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0, steps = pre + T;
    auto hour_of = [pre](int s) { return s < pre ? s : s - pre; };

    const bool sparse = pl.sparse;  // (with grad_dest: the tangent is the compact one, grad_batch_plan has checked it)
    const int *const d_ell = sparse ? c->d_exps_ell.get() : c->d_exp_ell.get();
    const double *const d_r = sparse ? c->d_exps_r.get() : c->d_exp_r.get();
    bool have_mu = gnext != nullptr;  // (false: zero by construction, the products of the last operator are skipped for every fleet)
    for (int s = steps - 1; s >= 0; --s) {
        const int t = hour_of(s), j = s - pre;
        const size_t row = static_cast<size_t>(t) * Z;
        const double *p_t = sparse ? nullptr : c->d_p + row * Z, *dp_t = grad_dest && !sparse ? c->d_tan + row * Z : nullptr;
        const int acc = s < pre ? 1 : 0;
        for (int f0 = 0; f0 < B; f0 += cpm::kExpMaxNB) {
            const int nf = std::min(B - f0, cpm::kExpMaxNB);
            const int NB = nf > 4 ? 8 : nf > 2 ? 4 : nf > 1 ? 2 : 1;
            const size_t w0 = static_cast<size_t>(f0) * Zs;
            const bool first = s == steps - 1;  // mu is G_next, as the caller laid it out
            const double *mu = !have_mu ? nullptr : (first && nf == 1) ? gnext + static_cast<size_t>(f0) * Z : ws_mu[(s + 1) & 1] + w0;
            const double *q_t = pd + f0 * q_stride + row;
            const double *pi_s = ws_pi + static_cast<size_t>(s) * nb * Zs + w0;
            const double *gp = j >= 0 ? cot + f0 * cot_stride + static_cast<size_t>(j) * Z : nullptr;
            const double *gd = j >= 0 ? gp + zt : nullptr;
            double *grad_t = grad_pd + f0 * zt + row, *dest_t = grad_dest ? grad_dest + f0 * zt + row : nullptr;
            const bool to_pi0 = s == 0 && grad_pi0;
            double *mu_out = to_pi0 ? grad_pi0 + static_cast<size_t>(f0) * Z : ws_mu[s & 1] + w0;
            if (nf == 1) {  // the B = 1 kernels: mu is one vector, the segments' sums are [nseg][Zs]
                if (mu) {
                    const dim3 grid(nblk(Z, cpm::kGradStrip), static_cast<unsigned>(nseg)), block(cpm::kExpBlock);
                    if (sparse) {
                        if (dest_t) launch_exps_grad_dest_u(c, row, mu, Zs, nseg, seg_len, part, part_dp);
                        else launch_exps_grad_u(c, row, mu, Zs, nseg, seg_len, part);
                    } else if (dp_t) {
                        if (Z & 1) cpm::launch(cpm::k_exp_grad_dest_u<true>, grid, block, 0, c->stream, p_t, dp_t, mu, Z, Zs, seg_len, part, part_dp);
                        else cpm::launch(cpm::k_exp_grad_dest_u<false>, grid, block, 0, c->stream, p_t, dp_t, mu, Z, Zs, seg_len, part, part_dp);
                    } else {
                        if (Z & 1) cpm::launch(cpm::k_exp_grad_u<true>, grid, block, 0, c->stream, p_t, mu, Z, Zs, seg_len, part);
                        else cpm::launch(cpm::k_exp_grad_u<false>, grid, block, 0, c->stream, p_t, mu, Z, Zs, seg_len, part);
                    }
                }
                if (dest_t) cpm::launch(cpm::k_exp_grad_dest_finish, dim3(nblk(Z, cpm::kFinishBlock)), dim3(cpm::kFinishBlock), 0, c->stream, part, part_dp, nseg, Zs,
                                        c->d_last + row, d_ell + row, d_r + row, q_t, pi_s, mu, gp, gd, Z, acc, mu_out, grad_t, dest_t);
                else cpm::launch(cpm::k_exp_grad_finish, dim3(nblk(Z, cpm::kFinishBlock)), dim3(cpm::kFinishBlock), 0, c->stream, part, nseg, Zs, c->d_last + row,
                                 d_ell + row, d_r + row, q_t, pi_s, mu, gp, gd, Z, acc, mu_out, grad_t);
                continue;
            }
            if (mu) {
                if (first) {
                    double *packed = ws_mu[(s + 1) & 1] + w0;
                    cpm::launch(cpm::k_exp_grad_pack_b, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(NB)), dim3(cpm::kExpBlock), 0, c->stream,
                                gnext + static_cast<size_t>(f0) * Z, Z, NB, nf, packed);
                }
                if (sparse && dest_t) {
                    using Gd = void (*)(cpm_ctx *, size_t, const double *, int, int, int, int, double *, double *);
                    const Gd gd_b = NB == 8 ? Gd(launch_exps_grad_dest_u_b<8>) : NB == 4 ? Gd(launch_exps_grad_dest_u_b<4>) : Gd(launch_exps_grad_dest_u_b<2>);
                    gd_b(c, row, mu, Zs, nseg, seg_len, nf, part, part_dp);
                } else if (sparse) {
                    using Gs = void (*)(cpm_ctx *, size_t, const double *, int, int, int, int, double *);
                    const Gs gs = NB == 8 ? Gs(launch_exps_grad_u_b<8>) : NB == 4 ? Gs(launch_exps_grad_u_b<4>) : Gs(launch_exps_grad_u_b<2>);
                    gs(c, row, mu, Zs, nseg, seg_len, nf, part);
                } else {
                    using Go = void (*)(cpm_ctx *, const double *, const double *, const double *, int, int, int, int, double *, double *);
                    const Go go = NB == 8 ? Go(launch_grad_u_b<8>) : NB == 4 ? Go(launch_grad_u_b<4>) : Go(launch_grad_u_b<2>);
                    go(c, p_t, dp_t, mu, Zs, nseg, seg_len, nf, part, part_dp);
                }
            }
            const dim3 grid(nblk(Z, cpm::kFinishBlock), static_cast<unsigned>(NB)), block(cpm::kFinishBlock);
            const size_t mo_o = to_pi0 ? 1 : static_cast<size_t>(NB), mo_f = to_pi0 ? static_cast<size_t>(Z) : 1;
            const int fill = to_pi0 ? 0 : 1;
            if (dest_t) cpm::launch(cpm::k_exp_grad_dest_finish_b, grid, block, 0, c->stream, part, part_dp, nseg, Zs, c->d_last + row, d_ell + row,
                                    d_r + row, q_t, q_stride, pi_s, mu, NB, gp, gd, cot_stride, Z, nf, acc, mu_out, mo_o, mo_f, fill, grad_t, dest_t, zt);
            else cpm::launch(cpm::k_exp_grad_finish_b, grid, block, 0, c->stream, part, nseg, Zs, c->d_last + row, d_ell + row, d_r + row, q_t,
                             q_stride, pi_s, mu, NB, gp, gd, cot_stride, Z, nf, acc, mu_out, mo_o, mo_f, fill, grad_t, zt);
        }
        HIP_TRY(hipGetLastError());
        have_mu = true;
    }
    return CPM_OK;
}

int32_t expected_grad_batch_enqueue(cpm_ctx *c, const double *d_pi0, uint32_t flags, int B, const double *pd, size_t q_stride, const double *cot,
                                    const double *gnext, double *grad_pd, double *grad_pi0, double *grad_dest, bool sparse = false)
{
    GradBatchPlan pl;
    int32_t rc = grad_batch_plan(c, B, grad_dest != nullptr, pl, sparse);
    if (rc != CPM_OK) return rc;
    if ((rc = grad_batch_forward(c, pl, d_pi0, flags, B, pd, q_stride)) != CPM_OK) return rc;
    return grad_batch_backward(c, pl, flags, B, pd, q_stride, cot, gnext, grad_pd, grad_pi0, grad_dest);
}

// the blocking forms: d_exp_gio holds [B][2][T][Z] cotangents, [B][Z] G_next, [B][T][Z] grad_p_drive, [B][Z] grad_pi0 and pi_0 [Z];
// d_exp_gdio [B][T][Z] grad_dest.  what: the entry, as its error text names it.
int32_t expected_grad_batch_blocking(cpm_ctx *c, const char *what, const double *pi0, uint32_t flags, int B, const double *pd, size_t q_stride,
                                     const double *g_parking, const double *g_driving, const double *g_next, double *grad_pd, double *grad_pi0, double *grad_dest,
                                     bool sparse = false)
{
    const size_t Z = static_cast<size_t>(c->Z), zt = Z * static_cast<size_t>(c->T), nb = static_cast<size_t>(B);
    int32_t rc = check_pi0(c, pi0);
    if (rc != CPM_OK) return rc;
    for (size_t i = 0; i < nb * zt; ++i)
        if (!std::isfinite(g_parking[i]) || !std::isfinite(g_driving[i]))
            return fail(CPM_ERR_ARG, "%s: the cotangent of fleet %lld, zone %lld, hour %lld is not finite", what, (long long)(i / zt) + 1, (long long)(i % Z) + 1,
                        (long long)(i % zt / Z) + 1);
    if (g_next)
        for (size_t i = 0; i < nb * Z; ++i)
            if (!std::isfinite(g_next[i]))
                return fail(CPM_ERR_ARG, "%s: g_next of fleet %lld, zone %lld is not finite", what, (long long)(i / Z) + 1, (long long)(i % Z) + 1);
    HIP_TRY(c->d_exp_gio.reserve(nb * (3 * zt + 2 * Z) + Z));
    if (grad_dest) HIP_TRY(c->d_exp_gdio.reserve(nb * zt));
    double *d_cot = c->d_exp_gio, *d_gnext = d_cot + nb * 2 * zt, *d_grad = d_gnext + nb * Z, *d_gpi0 = d_grad + nb * zt, *d_pi0 = d_gpi0 + nb * Z;
    for (size_t b = 0; b < nb; ++b) {
        HIP_TRY(hipMemcpyAsync(d_cot + b * 2 * zt, g_parking + b * zt, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_cot + b * 2 * zt + zt, g_driving + b * zt, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
    }
    if (g_next) HIP_TRY(hipMemcpyAsync(d_gnext, g_next, sizeof(double) * nb * Z, hipMemcpyHostToDevice, c->stream));
    if (pi0) HIP_TRY(hipMemcpyAsync(d_pi0, pi0, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    rc = expected_grad_batch_enqueue(c, pi0 ? d_pi0 : nullptr, flags, B, pd, q_stride, d_cot, g_next ? d_gnext : nullptr, d_grad, grad_pi0 ? d_gpi0 : nullptr,
                                     grad_dest ? c->d_exp_gdio.get() : nullptr, sparse);
    if (rc != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(grad_pd, d_grad, sizeof(double) * nb * zt, hipMemcpyDeviceToHost, c->stream));
    if (grad_pi0) HIP_TRY(hipMemcpyAsync(grad_pi0, d_gpi0, sizeof(double) * nb * Z, hipMemcpyDeviceToHost, c->stream));
    if (grad_dest) HIP_TRY(hipMemcpyAsync(grad_dest, c->d_exp_gdio, sizeof(double) * nb * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// d p_destin / d e_dest of the installed tables into d_tan (enqueued on the context's stream): from the compact rows when the tables
// are the dataset route's, else from the datamatrix and the dense p_destin array.
int32_t build_dest_tangent(cpm_ctx *c)
{
    if (!c->have_cdf || !c->dest_built)
        return fail(CPM_ERR_STATE, "build_p_dest_tangent: the installed p_destin tables do not come from cpm_build_p_dest on the resident datamatrix");
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "build_p_dest_tangent: no datamatrix is resident");
    if (!(c->dest_built_e > 0.0)) return fail(CPM_ERR_STATE, "build_p_dest_tangent: the tables were built with e_dest = %g; the tangent needs e_dest > 0", c->dest_built_e);
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t cells = static_cast<size_t>(Z) * Z * T;
    c->tan_valid = false;
    HIP_TRY(c->d_tan.reserve(cells));
    if (c->sparse_tables) {
        if (c->tables_uploaded || !c->ds_valid || !c->ds_ok)
            return fail(CPM_ERR_STATE, "build_p_dest_tangent: the compact rows these tables were built from are gone");
        const int64_t rows = c->T * c->Z;
        HIP_TRY(hipMemsetAsync(c->d_tan, 0, sizeof(double) * cells, c->stream));
        cpm::launch(cpm::k_tan_cells, dim3(nblk(rows, 64)), dim3(64), 0, c->stream, c->d_ds_cells.get(), c->d_sp.get(), c->d_sj.get(), c->d_scnt.get(),
                    cpm::kDsCap, rows, Z, c->d_tan.get());
        HIP_TRY(hipGetLastError());
    } else {
        if (!c->d_p) return fail(CPM_ERR_STATE, "build_p_dest_tangent: p_dest not set");
        HIP_TRY(c->d_tan_m.reserve(static_cast<size_t>(Z) * T));
        const dim3 g1(nblk(Z, 256), static_cast<unsigned>(Z));
        if (T == 24) cpm::launch(cpm::k_tan_log<24>, g1, dim3(256), 0, c->stream, c->d_dm.get(), c->d_p.get(), c->d_tan.get(), Z, T);
        else cpm::launch(cpm::k_tan_log<0>, g1, dim3(256), 0, c->stream, c->d_dm.get(), c->d_p.get(), c->d_tan.get(), Z, T);
        HIP_TRY(hipGetLastError());
        cpm::launch(cpm::k_tan_rowsum, dim3(nblk(Z, 64), static_cast<unsigned>(T)), dim3(64), 0, c->stream, c->d_p.get(), c->d_tan.get(), c->d_tan_m.get(), Z);
        HIP_TRY(hipGetLastError());
        cpm::launch(cpm::k_tan_final, dim3(nblk(Z, 256), nblk(Z, cpm::kDivBatch), static_cast<unsigned>(T)), dim3(256), 0, c->stream, c->d_p.get(),
                    c->d_tan_m.get(), c->d_tan.get(), Z);
        HIP_TRY(hipGetLastError());
    }
    c->tan_valid = true;
    ++c->tan_gen;
    return CPM_OK;
}

// the tangent of the trip weights into d_dw [2][T][Z] (enqueued): k_exp_trip on the tangent table, then the segments in order
int32_t trip_tangent_enqueue(cpm_ctx *c, double *d_dw)
{
    int32_t rc = exp_tables_ready(c, "expected_trip_tangent");
    if (rc != CPM_OK) return rc;
    if ((rc = tangent_ready(c, "expected_trip_tangent")) != CPM_OK) return rc;
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "expected_trip_tangent: datamatrix not set (cpm_set_datamatrix, cpm_createdatamatrix_* or cpm_synth_datamatrix)");
    if (!c->have_dist) return fail(CPM_ERR_STATE, "expected_trip_tangent: distance matrix not set (cpm_set_distance* or the dist of cpm_set_datamatrix)");
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t zt = static_cast<size_t>(Z) * T;
    const int nseg = cpm::trip_segments(Z, T), seg_len = cpm::trip_segment_len(Z, nseg);
    HIP_TRY(c->d_exp_wpart.reserve(2 * zt * nseg));  // (scratch of the trip weights' own build: nothing reads it afterwards)
    const dim3 grid(nblk(Z, cpm::kTripStrip), static_cast<unsigned>(T), static_cast<unsigned>(nseg));
    if (Z & 1) cpm::launch(cpm::k_exp_trip<true>, grid, dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(c->d_tan.get()),
                           static_cast<const double *>(c->d_dm.get()), static_cast<const double *>(c->d_dist.get()), Z, T, seg_len, c->d_exp_wpart.get());
    else cpm::launch(cpm::k_exp_trip<false>, grid, dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(c->d_tan.get()),
                     static_cast<const double *>(c->d_dm.get()), static_cast<const double *>(c->d_dist.get()), Z, T, seg_len, c->d_exp_wpart.get());
    HIP_TRY(hipGetLastError());
    cpm::launch(cpm::k_exp_trip_tan_finish, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T)), dim3(cpm::kExpBlock), 0, c->stream,
                static_cast<const double *>(c->d_exp_wpart.get()), nseg, static_cast<const double *>(c->d_last), Z, T, d_dw);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

// ... from the compact tangent (include/cpm_expected_sparse_dest.h): k_exps_trip on the rows of d_sdp in place of those of d_sp, then
// the same finishing kernel.  Neither d_p nor d_tan is read.
int32_t trip_tangent_sparse_enqueue(cpm_ctx *c, double *d_dw)
{
    int32_t rc = exp_tables_ready(c, "expected_sparse_trip_tangent");
    if (rc != CPM_OK) return rc;
    if (!c->sparse_tables) return exps_no_rows();
    if ((rc = sdp_ready(c, "expected_sparse_trip_tangent")) != CPM_OK) return rc;
    if (!c->have_dmat)
        return fail(CPM_ERR_STATE, "expected_sparse_trip_tangent: datamatrix not set (cpm_set_datamatrix, cpm_createdatamatrix_* or cpm_synth_datamatrix)");
    if (!c->have_dist) return fail(CPM_ERR_STATE, "expected_sparse_trip_tangent: distance matrix not set (cpm_set_distance* or the dist of cpm_set_datamatrix)");
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t zt = static_cast<size_t>(Z) * T;
    const int nseg = cpm::trip_segments(Z, T), seg_len = cpm::trip_segment_len(Z, nseg);
    HIP_TRY(c->d_exp_wpart.reserve(2 * zt * nseg));  // (scratch of the trip weights' own build: nothing reads it afterwards)
    cpm::launch(cpm::k_exps_trip, dim3(static_cast<unsigned>(Z), static_cast<unsigned>(T)), dim3(cpm::kExpsGradBlock), 0, c->stream,
                static_cast<const double *>(c->d_sdp.get()), static_cast<const uint32_t *>(c->d_sj.get()), static_cast<const uint32_t *>(c->d_scnt.get()),
                cpm::kDsCap, static_cast<const double *>(c->d_dm.get()), static_cast<const double *>(c->d_dist.get()), Z, T, seg_len, nseg,
                c->d_exp_wpart.get());
    HIP_TRY(hipGetLastError());
    cpm::launch(cpm::k_exp_trip_tan_finish, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T)), dim3(cpm::kExpBlock), 0, c->stream,
                static_cast<const double *>(c->d_exp_wpart.get()), nseg, static_cast<const double *>(c->d_last), Z, T, d_dw);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

// ------------------------------------------------------------------ value and gradient of the objectives (include/cpm_expected_fit.h)
constexpr int kFitMaxT = 2048;  // (the hours' sums of a workgroup live in LDS; an argmin and an argmax share a word)

// what every entry checks before anything is enqueued, behind exp_enter; B and the parameter arrays included
int32_t fit_check(cpm_ctx *c, const char *what, int32_t B, const double *p_min, const double *p_max, const double *e_drive, uint32_t flags, const double *weights,
                  const void *record, bool sparse = false)
{
    if (B < 1 || B > CPM_MAX_BATCH) return fail(CPM_ERR_ARG, "%s: B = %d outside 1..%d", what, B, CPM_MAX_BATCH);
    if (!p_min || !p_max || !e_drive) return fail(CPM_ERR_ARG, "%s: null parameter array", what);
    if (!weights) return fail(CPM_ERR_ARG, "%s: null weights", what);
    if (!record) return fail(CPM_ERR_ARG, "%s: null record", what);
    if (flags & ~(CPM_EXPECT_IVP | CPM_FIT_DEST)) return fail(CPM_ERR_ARG, "%s: unknown flag bits 0x%x", what, flags);
    for (int i = 0; i < 3 * B; ++i)
        if (!std::isfinite(weights[i])) return fail(CPM_ERR_ARG, "%s: weight %d of fleet %d is not finite", what, i % 3 + 1, i / 3 + 1);
    CTX_TRY(c);
    if (c->T > kFitMaxT) return fail(CPM_ERR_ARG, "%s: T = %lld above %d", what, (long long)c->T, kFitMaxT);
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "%s: datamatrix not set (cpm_set_datamatrix, cpm_createdatamatrix_* or cpm_synth_datamatrix)", what);
    if (!c->have_dist) return fail(CPM_ERR_STATE, "%s: distance matrix not set (cpm_set_distance* or the dist of cpm_set_datamatrix)", what);
    int32_t rc = exp_tables_ready(c, what);
    if (rc != CPM_OK) return rc;
    if ((flags & CPM_FIT_DEST) && (rc = sparse ? sdp_ready(c, what) : tangent_ready(c, what)) != CPM_OK) return rc;
    for (int b = 0; b < B; ++b) {
        if (weights[3 * b] != 0.0 && !c->have_act_meas)
            return fail(CPM_ERR_STATE, "%s: fleet %d weighs activity_error, but no measured activity is installed (cpm_set_measured_activity)", what, b + 1);
        if (weights[3 * b + 1] != 0.0 && !c->have_measured)
            return fail(CPM_ERR_STATE, "%s: fleet %d weighs parking_error, but no measured parking densities are installed (cpm_set_measured)", what, b + 1);
    }
    return CPM_OK;
}

// where the call's arrays lie in d_fit_ws
struct FitLayout {
    size_t expected, cot, grad_pd, grad_dest, params, totals, ga, nval, hpart, epart, zone, range, cpart, words;
    int nbz, nchunk;
};
FitLayout fit_layout(const cpm_ctx *c, int B)
{
    const size_t nb = static_cast<size_t>(B), Z = static_cast<size_t>(c->Z), T = static_cast<size_t>(c->T), zt = Z * T;
    FitLayout l;
    l.nbz = static_cast<int>(nblk(c->Z, cpm::kExpBlock));
    l.nchunk = static_cast<int>(nblk(static_cast<int64_t>(zt), cpm::kTravelChunk));
    size_t at = 0;
    auto take = [&at](size_t n) { const size_t here = at; at += (n + 1) & ~static_cast<size_t>(1); return here; };
    l.expected = take(nb * 2 * zt);
    l.cot = take(nb * 2 * zt);
    l.grad_pd = take(nb * zt);
    l.grad_dest = take(nb * zt);
    l.zone = take(5 * nb * Z);
    l.range = take(2 * Z);
    l.hpart = take(nb * T * l.nbz);
    l.epart = take(nb * l.nbz);
    l.cpart = take(nb * l.nchunk * cpm::kFitChainTerms);
    l.ga = take(nb * T);
    l.params = take(6 * nb);
    l.totals = take(2 * nb);
    l.nval = take(nb);
    l.words = at;
    return l;
}

// The whole call, enqueued on the context's stream; fit_check has passed.  Outputs that are nullptr stay in the workspace.
// sparse: the propagation, the trip weights (d_exps_w) and the adjoint read the compact rows, CPM_FIT_DEST the compact tangent (the
// entries refuse it where none is installed).
int32_t expected_fit_enqueue(cpm_ctx *c, int B, const double *p_min, const double *p_max, const double *e_drive, const double *d_pi0, uint32_t flags,
                             const double *weights, double *d_record, double *d_expected, double *d_cot, double *d_grad_pd, double *d_grad_dest,
                             bool sparse = false)
{
    const bool dest = (flags & CPM_FIT_DEST) != 0;
    const uint32_t eflags = flags & CPM_EXPECT_IVP;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t zt = static_cast<size_t>(Z) * T;
    GradBatchPlan pl;
    int32_t rc = grad_batch_plan(c, B, dest, pl, sparse);
    if (rc != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps_trip(c) : ensure_exp_trip(c)) != CPM_OK) return rc;
    bool direct = false;
    for (int b = 0; b < B; ++b) direct = direct || (dest && weights[3 * b + 2] != 0.0);
    if (direct && !sparse && (c->fit_dw_gen != c->tan_gen || c->fit_dw_builds != c->exp_trip_builds)) {
        c->fit_dw_gen = -1;
        HIP_TRY(c->d_fit_dw.reserve(2 * zt));
        if ((rc = trip_tangent_enqueue(c, c->d_fit_dw)) != CPM_OK) return rc;
        c->fit_dw_gen = c->tan_gen;
        c->fit_dw_builds = c->exp_trip_builds;
    }
    if (direct && sparse && (c->fits_dw_gen != c->sdp_gen || c->fits_dw_builds != c->exps_trip_builds)) {  // (a cache of its own, as d_exps_w is)
        c->fits_dw_gen = -1;
        HIP_TRY(c->d_fits_dw.reserve(2 * zt));
        if ((rc = trip_tangent_sparse_enqueue(c, c->d_fits_dw)) != CPM_OK) return rc;
        c->fits_dw_gen = c->sdp_gen;
        c->fits_dw_builds = c->exps_trip_builds;
    }
    if ((rc = ensure_batch_tables(c, B)) != CPM_OK) return rc;
    if ((rc = ensure_pdrive_mean(c)) != CPM_OK) return rc;
    const FitLayout l = fit_layout(c, B);
    HIP_TRY(c->d_fit_ws.reserve(l.words));  // (a grow frees first: hipFree waits for what still reads the old workspace)
    HIP_TRY(c->d_fit_int.reserve(static_cast<size_t>(B) * (Z + l.nbz)));
    double *ws = c->d_fit_ws;
    double *expected = d_expected ? d_expected : ws + l.expected, *cot = d_cot ? d_cot : ws + l.cot;
    double *grad_pd = d_grad_pd ? d_grad_pd : ws + l.grad_pd;
    double *grad_dest = !dest ? nullptr : d_grad_dest ? d_grad_dest : ws + l.grad_dest;
    double *w_dev = ws + l.params, *par_dev = w_dev + 3 * B;
    int *arg = c->d_fit_int, *npart = arg + static_cast<size_t>(B) * Z;
    const size_t rec_stride = static_cast<size_t>(cpm::kFitWords + T);

    // (a) the B tables, as cpm_build_p_drive_batch installs them
    for (int b = 0; b < B; ++b)
        hipLaunchKernelGGL(cpm::k_pdrive_final, dim3(nblk(c->Z, 64), static_cast<unsigned>(c->T)), dim3(64), 0, c->stream, c->d_pdrive_mean,
                           c->d_pdrive_b + b * zt, c->d_thr_b + b * zt, Z, T, p_min[b], p_max[b], e_drive[b]);
    HIP_TRY(hipGetLastError());
    c->batch_B = B;
    cpm::FitParams fp;
    for (int b = 0; b < B; ++b) {
        fp.w[3 * b] = weights[3 * b], fp.w[3 * b + 1] = weights[3 * b + 1], fp.w[3 * b + 2] = weights[3 * b + 2];
        fp.w[3 * (B + b)] = p_min[b], fp.w[3 * (B + b) + 1] = p_max[b], fp.w[3 * (B + b) + 2] = e_drive[b];
    }
    hipLaunchKernelGGL(cpm::k_fit_params, dim3(1), dim3(64), 0, c->stream, fp, 6 * B, w_dev);
    HIP_TRY(hipGetLastError());

    // (b) forward, pi_s kept; the densities of the day from them
    const double *pd = c->d_pdrive_b;
    if ((rc = grad_batch_forward(c, pl, d_pi0, eflags, B, pd, zt)) != CPM_OK) return rc;
    const int pre = (eflags & CPM_EXPECT_IVP) ? T - 1 : 0;
    const unsigned nbz = static_cast<unsigned>(l.nbz);
    hipLaunchKernelGGL(cpm::k_fit_dens, dim3(nbz, static_cast<unsigned>(T), static_cast<unsigned>(B)), dim3(cpm::kExpBlock), 0, c->stream,
                       static_cast<const double *>(pl.ws_pi + static_cast<size_t>(pre) * pl.nb * pl.Zs), pd, zt, Z, pl.Zs, T, B, expected);
    HIP_TRY(hipGetLastError());

    // (c) objectives and cotangents
    if ((rc = expected_travel_enqueue(c, expected, B, nullptr, ws + l.totals, sparse)) != CPM_OK) return rc;
    const double *meas = c->have_measured ? c->d_measured.get() : nullptr;
    const int *flag = c->have_measured ? c->d_meas_flag.get() : nullptr;
    hipLaunchKernelGGL(cpm::k_fit_zones, dim3(nbz, static_cast<unsigned>(B)), dim3(cpm::kExpBlock), sizeof(double) * cpm::kExpWaves * T, c->stream,
                       static_cast<const double *>(expected), meas, flag, Z, T, B, ws + l.hpart, ws + l.zone, arg, ws + l.epart, npart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cpm::k_fit_final, dim3(static_cast<unsigned>(B)), dim3(64), sizeof(double) * T, c->stream, static_cast<const double *>(ws + l.hpart),
                       static_cast<const double *>(ws + l.epart), static_cast<const int *>(npart), l.nbz, T, static_cast<const double *>(ws + l.totals),
                       c->have_act_meas ? static_cast<const double *>(c->d_act_meas.get()) : nullptr, static_cast<const double *>(w_dev), d_record, rec_stride,
                       ws + l.ga, ws + l.nval);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cpm::k_fit_cot, dim3(nbz, static_cast<unsigned>(B)), dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(expected), meas,
                       static_cast<const double *>(ws + l.zone), static_cast<const int *>(arg), static_cast<const double *>(ws + l.ga),
                       static_cast<const double *>(ws + l.nval), static_cast<const double *>(sparse ? c->d_exps_w.get() : c->d_exp_w.get()),
                       static_cast<const double *>(w_dev), Z, T, B, cot);
    HIP_TRY(hipGetLastError());

    // (d) backward on that cotangent: G_next zero, grad_pi0 not wanted
    if ((rc = grad_batch_backward(c, pl, eflags, B, pd, zt, cot, nullptr, grad_pd, nullptr, grad_dest)) != CPM_OK) return rc;

    // (e) the chain rule
    hipLaunchKernelGGL(cpm::k_fit_mean_range, dim3(nbz), dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(c->d_pdrive_mean.get()), Z, T,
                       ws + l.range);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cpm::k_fit_chain, dim3(static_cast<unsigned>(l.nchunk), static_cast<unsigned>(B)), dim3(cpm::kExpBlock), 0, c->stream,
                       static_cast<const double *>(grad_pd), static_cast<const double *>(grad_dest), static_cast<const double *>(expected),
                       direct ? static_cast<const double *>(sparse ? c->d_fits_dw.get() : c->d_fit_dw.get()) : nullptr,
                       static_cast<const double *>(c->d_pdrive_mean.get()),
                       static_cast<const double *>(ws + l.range), static_cast<const double *>(par_dev), static_cast<const double *>(w_dev), Z, zt, ws + l.cpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cpm::k_fit_chain_total, dim3(static_cast<unsigned>(B)), dim3(64), 0, c->stream, static_cast<const double *>(ws + l.cpart), l.nchunk,
                       static_cast<const double *>(w_dev), dest ? 1 : 0, T, d_record, rec_stride);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

// ------------------------------------------------------------------ forward tangent of the expected densities (include/cpm_expected_tangent.h)
// what every entry checks behind exp_enter, before anything is read, copied or enqueued
int32_t tangent_check(cpm_ctx *c, const char *what, int32_t K, uint32_t flags, const double *c_dest, const void *out, bool sparse = false)
{
    if (K < 1 || K > CPM_TANGENT_MAX_DIRECTIONS) return fail(CPM_ERR_ARG, "%s: K = %d outside 1 .. %d", what, K, CPM_TANGENT_MAX_DIRECTIONS);
    if (!out) return fail(CPM_ERR_ARG, "%s: null tangent output", what);
    int32_t rc = exp_flags_check(flags);
    if (rc != CPM_OK) return rc;
    bool any = false;
    if (c_dest)
        for (int k = 0; k < K; ++k) {
            if (!std::isfinite(c_dest[k])) return fail(CPM_ERR_ARG, "%s: c_dest of direction %d is not finite", what, k + 1);
            any = any || c_dest[k] != 0.0;
        }
    CTX_TRY(c);
    if (!c->have_pdrive) return fail(CPM_ERR_STATE, "%s: p_drive not set", what);
    if ((rc = exp_tables_ready(c, what)) != CPM_OK) return rc;
    if (sparse && !c->sparse_tables) return exps_no_rows();
    if (any && (rc = sparse ? sdp_ready(c, what) : tangent_ready(c, what)) != CPM_OK) return rc;
    return CPM_OK;
}

template <int NB>
void launch_tan_hour(cpm_ctx *c, const cpm::TanHour &a)
{
    cpm::launch(cpm::k_tan_hour<NB>, dim3(nblk(a.Z, cpm::kExpRows)), dim3(cpm::kExpBlock), 0, c->stream, a);
}

// the same operator from the transposed compact rows (k_exps_tan_hour; ensure_exps built them, ensure_exps_dp the tangent's cells)
template <int NB>
void launch_exps_tan_hour(cpm_ctx *c, const cpm::ExpsTanHour &b)
{
    const dim3 grid(nblk(b.h.Z, cpm::kExpRows)), block(cpm::kExpBlock);
    if (b.h.u_mode == 1) cpm::launch(cpm::k_exps_tan_hour<NB, true>, grid, block, 0, c->stream, b);
    else cpm::launch(cpm::k_exps_tan_hour<NB, false>, grid, block, 0, c->stream, b);
}

// The compact tangent in the transposed cell order (k_exps_cells_dp): once per compact tangent and table build.  Enqueued.
int32_t ensure_exps_dp(cpm_ctx *c)
{
    if (c->exps_dp_gen == c->sdp_gen && c->d_exps_dp) return CPM_OK;
    HIP_TRY(c->d_exps_dp.reserve(std::max<size_t>(c->exps_cells, 1)));
    cpm::launch(cpm::k_exps_cells_dp, dim3(static_cast<unsigned>(c->Z), static_cast<unsigned>(c->T)), dim3(cpm::kExpBlock), 0, c->stream,
                c->d_exps_colptr.get(), c->d_exps_o.get(), c->d_sdp.get(), c->d_sj.get(), c->d_scnt.get(), cpm::kDsCap, static_cast<int>(c->Z),
                c->d_exps_dp.get());
    HIP_TRY(hipGetLastError());
    c->exps_dp_gen = c->sdp_gen;
    return CPM_OK;
}

// The recurrence of expected_enqueue (B = 1, the installed p_drive) for the primal and K directions: operator-major, per operator one
// launch per pass of at most kTanDirs directions.  dpi0: [K][Z], dpd: [K][T][Z], c_dest: host [K] (each or nullptr: zero).
// out: [K][2][T][Z]; dpi_next: [K][Z] or nullptr; expected: [2][T][Z] or nullptr.
// sparse: the operators read the transposed compact rows and the compact tangent (k_exps_tan_hour) and the per-table arrays of ensure_exps.
int32_t expected_tangent_enqueue(cpm_ctx *c, int K, const double *d_pi0, uint32_t flags, const double *dpi0, const double *dpd, const double *c_dest,
                                 double *out, double *dpi_next, double *expected, bool sparse = false)
{
    int32_t rc = sparse ? ensure_exps(c) : ensure_exp_aux(c);
    if (rc != CPM_OK) return rc;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const int Zs = (Z + 1) & ~1;  // (every vector starts on a 16-byte line)
    const size_t zt = static_cast<size_t>(Z) * T;
    bool with_u = false;
    if (c_dest)
        for (int k = 0; k < K; ++k) with_u = with_u || c_dest[k] != 0.0;
    if (sparse && with_u) {
        if ((rc = sdp_ready(c, "expected_sparse_tangent")) != CPM_OK) return rc;
        if ((rc = ensure_exps_dp(c)) != CPM_OK) return rc;
    }
    const int npass = (K + cpm::kTanDirs - 1) / cpm::kTanDirs;
    const size_t side = static_cast<size_t>(npass) * 2 * cpm::kExpMaxNB * Zs;   // [passes][pi | x][8][Zs]
    HIP_TRY(c->d_tanf_ws.reserve(2 * side + 3 * static_cast<size_t>(Zs)));  // (a grow frees first: hipFree waits for what still reads the old workspace)
    double *ws[2] = {c->d_tanf_ws, c->d_tanf_ws + side};
    double *ws_xm[2] = {c->d_tanf_ws + 2 * side, c->d_tanf_ws + 2 * side + Zs};
    double *ws_u = c->d_tanf_ws + 2 * side + 2 * static_cast<size_t>(Zs);
    const size_t vec = static_cast<size_t>(cpm::kExpMaxNB) * Zs;
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0;  // operators in front of the day
    const double *pd = c->d_pdrive;
    for (int ps = 0; ps < npass; ++ps) {
        const int k0 = ps * cpm::kTanDirs, nv = std::min(K - k0, cpm::kTanDirs) + 1;
        double *pi = ws[0] + static_cast<size_t>(ps) * 2 * vec;
        double *dpark = pre == 0 ? out + static_cast<size_t>(k0) * 2 * zt : nullptr;
        cpm::launch(cpm::k_tan_init, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(nv)), dim3(cpm::kExpBlock), 0, c->stream, d_pi0,
                    dpi0 ? dpi0 + static_cast<size_t>(k0) * Z : nullptr, pd, dpd ? dpd + static_cast<size_t>(k0) * zt : nullptr, zt,
                    static_cast<const double *>(c->d_last), Z, Zs, pi, pi + vec, (ps == 0 && with_u) ? ws_xm[0] : nullptr,
                    (ps == 0 && pre == 0) ? expected : nullptr, (ps == 0 && pre == 0 && expected) ? expected + zt : nullptr, dpark,
                    dpark ? dpark + zt : nullptr, 2 * zt);
    }
    HIP_TRY(hipGetLastError());
    const int steps = pre + T;
    for (int s = 0; s < steps; ++s) {
        const int t = s < pre ? s : s - pre;
        const int day_next = s + 1 - pre;  // the hour of the day whose state this step produces (< 0: still in front of it)
        const bool more = s + 1 < steps;
        const int t_next = s + 1 < pre ? s + 1 : s + 1 - pre;
        const int in = s & 1, ot = in ^ 1;
        const size_t row = static_cast<size_t>(t) * Z;
        for (int ps = 0; ps < npass; ++ps) {
            const int k0 = ps * cpm::kTanDirs, nv = std::min(K - k0, cpm::kTanDirs) + 1;
            cpm::TanHour a{};
            a.p_t = sparse ? nullptr : c->d_p + row * Z;
            a.last_t = c->d_last + row;
            a.r_t = (sparse ? c->d_exps_r : c->d_exp_r) + row;
            a.start_t = (sparse ? c->d_exps_start : c->d_exp_start) + static_cast<size_t>(t) * (Z + 1);
            a.list_t = (sparse ? c->d_exps_list : c->d_exp_list) + row;
            a.last_next = more ? c->d_last + static_cast<size_t>(t_next) * Z : nullptr;
            a.dp_t = (with_u && !sparse) ? c->d_tan + row * Z : nullptr;
            a.u = ws_u;
            a.u_mode = !with_u ? 0 : ps == 0 ? 1 : 2;
            a.q_cur = pd + row;
            a.q_next = more ? pd + static_cast<size_t>(t_next) * Z : nullptr;
            a.dq_cur = dpd ? dpd + static_cast<size_t>(k0) * zt + row : nullptr;
            a.dq_next = (dpd && more) ? dpd + static_cast<size_t>(k0) * zt + static_cast<size_t>(t_next) * Z : nullptr;
            a.dq_stride = zt;
            a.pi_in = ws[in] + static_cast<size_t>(ps) * 2 * vec;
            a.x_in = a.pi_in + vec;
            a.xm_in = ws_xm[in];
            a.pi_out = ws[ot] + static_cast<size_t>(ps) * 2 * vec;
            a.x_out = a.pi_out + vec;
            a.xm_out = (ps == 0 && with_u && more) ? ws_xm[ot] : nullptr;
            if (day_next >= 0 && day_next < T) {
                a.dpark = out + static_cast<size_t>(k0) * 2 * zt + static_cast<size_t>(day_next) * Z;
                a.ddrv = a.dpark + zt;
                a.out_stride = 2 * zt;
                if (ps == 0 && expected) {
                    a.park0 = expected + static_cast<size_t>(day_next) * Z;
                    a.drv0 = a.park0 + zt;
                }
            } else if (day_next == T && dpi_next) {
                a.dpark = dpi_next + static_cast<size_t>(k0) * Z;
                a.out_stride = static_cast<size_t>(Z);
            }
            for (int f = 1; f < nv; ++f) a.c[f] = c_dest ? c_dest[k0 + f - 1] : 0.0;
            a.Z = Z;
            a.Zs = Zs;
            a.nv = nv;
            // the smallest instantiation that holds the pass (vectors beyond nv repeat the last one and are not stored)
            if (sparse) {
                cpm::ExpsTanHour b{};
                b.h = a;
                b.colptr_t = c->d_exps_colptr + static_cast<size_t>(t) * (Z + 1);
                b.cell_o = c->d_exps_o.get();
                b.cell_p = c->d_exps_p.get();
                b.cell_dp = with_u ? c->d_exps_dp.get() : nullptr;
                b.par = t & 1;
                if (nv > 5) launch_exps_tan_hour<8>(c, b);
                else if (nv > 4) launch_exps_tan_hour<5>(c, b);
                else if (nv > 2) launch_exps_tan_hour<4>(c, b);
                else launch_exps_tan_hour<2>(c, b);
            } else if (nv > 5) launch_tan_hour<8>(c, a);
            else if (nv > 4) launch_tan_hour<5>(c, a);  // (K = 4: the model's four parameters)
            else if (nv > 2) launch_tan_hour<4>(c, a);
            else launch_tan_hour<2>(c, a);
        }
        HIP_TRY(hipGetLastError());
    }
    return CPM_OK;
}

int32_t check_finite(const char *what, const char *name, const double *v, size_t n)
{
    if (v)
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(v[i])) return fail(CPM_ERR_ARG, "%s: word %zu of %s is not finite", what, i + 1, name);
    return CPM_OK;
}

// the builder of the three direction tables (cpm_expected_tangent.h): enqueued
int32_t pdrive_tangent_enqueue(cpm_ctx *c, double p_min, double p_max, double e_drive, double *d_out)
{
    if (!c->have_dm()) return fail(CPM_ERR_STATE, "build_p_drive_tangent: datamatrix and distance matrix first");
    int32_t rc = ensure_pdrive_mean(c);
    if (rc != CPM_OK) return rc;
    cpm::launch(cpm::k_tan_pdrive, dim3(nblk(c->Z, 64), static_cast<unsigned>(c->T)), dim3(64), 0, c->stream,
                static_cast<const double *>(c->d_pdrive_mean.get()), d_out, static_cast<int>(c->Z), static_cast<int>(c->T), p_min, p_max, e_drive);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

}  // namespace

extern "C" {

const char *cpm_last_error(void) { return g_last_error.c_str(); }

int32_t cpm_version(void) { return 100; }

int32_t cpm_device_count(int32_t *n_out)
{
    if (!n_out) return fail(CPM_ERR_ARG, "null n_out");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    *n_out = n;
    return CPM_OK;
}

int32_t cpm_device_info(int32_t device_id, char *name, int32_t len, int32_t *cu_count, int64_t *hbm_bytes)
{
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device_id));
    if (name && len > 0) {
        std::snprintf(name, static_cast<size_t>(len), "%s (%s)", p.name, p.gcnArchName);
    }
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = static_cast<int64_t>(p.totalGlobalMem);
    return CPM_OK;
}

int32_t cpm_create(cpm_ctx **ctx_out, int64_t Z, int64_t T, int32_t device_id)
{
    if (!ctx_out) return fail(CPM_ERR_ARG, "null ctx_out");
    *ctx_out = nullptr;
    if (Z < 1 || Z > (int64_t(1) << 24)) return fail(CPM_ERR_ARG, "number_zones %lld out of range", (long long)Z);
    if (T < 1 || T > 4096) return fail(CPM_ERR_ARG, "T %lld out of range", (long long)T);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(CPM_ERR_HIP, "no HIP device: this library has no CPU path");
    if (device_id < 0 || device_id >= ndev) return fail(CPM_ERR_ARG, "device %d of %d", device_id, ndev);
    HIP_TRY(hipSetDevice(device_id));
    cpm_ctx *c = new (std::nothrow) cpm_ctx();
    if (!c) return fail(CPM_ERR_NOMEM, "host allocation failed");
    c->Z = Z;
    c->T = T;
    c->Zp = static_cast<int>((Z + 15) / 16 * 16);
    c->Zq = cpm::pack_zq(static_cast<int>(Z));
    c->pk_G = cpm::pack_guide_bits(static_cast<int>(Z));
    c->pk_Zc = static_cast<int>(Z);
    c->device = device_id;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device_id) == hipSuccess) c->cu_count = p.multiProcessorCount;
    if (c->cu_count <= 0) c->cu_count = 256;
    hipError_t e = c->d_err.reserve(1);
    if (e == hipSuccess) e = hipMemset(c->d_err, 0, sizeof(int));
    if (e == hipSuccess) e = c->h_err.reserve(1);
    if (e == hipSuccess) e = c->d_counts.reserve(static_cast<size_t>(2 * T * Z + 2));
    if (e == hipSuccess) e = c->h_counts.reserve(static_cast<size_t>(2 * T * Z + 2));
    if (e == hipSuccess) e = c->h_status.reserve(2);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->status_ev, hipEventDisableTiming);
    if (e == hipSuccess) c->h_status[0] = c->h_status[1] = 0;
    if (e == hipSuccess) e = c->h_ivp_status.reserve(2);
    if (e == hipSuccess) c->h_ivp_status[0] = c->h_ivp_status[1] = 0;
    if (e != hipSuccess) {
        cpm_destroy(c);
        return fail(CPM_ERR_HIP, "context setup: %s", hipGetErrorString(e));
    }
#ifdef CPM_DEV_ENV  // development builds only (tools/build_variants.sh ... "-DCPM_DEV_ENV"): the product reads nothing from the environment
    if (const char *v = std::getenv("CPM_FUSED")) cpm_set_option(c, CPM_OPT_FUSED, std::atoi(v));
    if (const char *v = std::getenv("CPM_HEAVY_X")) c->zg.heavy_x_seen = static_cast<uint32_t>(std::max(1, std::min(16, std::atoi(v))));
    if (const char *v = std::getenv("CPM_FUSED_LAG")) cpm_set_option(c, CPM_OPT_FUSED_LAG, std::atoi(v));
#endif
    *ctx_out = c;
    return CPM_OK;
}

int32_t cpm_destroy(cpm_ctx *c)
{
    if (!c) return CPM_OK;
    (void)hipSetDevice(c->device);
    if (c->have_stream) (void)hipStreamSynchronize(c->stream);
    dfree(c->d_pdrive);  // the four that are re-pointed for a step or a launch, hence plain pointers (see cpm_ctx)
    dfree(c->d_thr);
    dfree(c->d_last);
    dfree(c->d_ckpt);
    c->zb.release();
    c->zx.release();
    c->zg.release();
    if (c->bstatus_ev) (void)hipEventDestroy(c->bstatus_ev);
    if (c->status_ev) (void)hipEventDestroy(c->status_ev);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;  // (every DevBuf / PinnedBuf member frees what it owns)
    return CPM_OK;
}

int32_t cpm_set_option(cpm_ctx *c, int32_t option, int64_t value)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");  // (host state only: no stream is needed, none is created)
    switch (option) {
    case CPM_OPT_KERNEL:
        if (value != CPM_KERNEL_AUTO && value != CPM_KERNEL_CAR && value != CPM_KERNEL_ZONE_LDS && value != CPM_KERNEL_ZONE_GROUPED) return fail(CPM_ERR_ARG, "unknown kernel %lld", (long long)value);
        c->kernel = static_cast<int>(value);
        return CPM_OK;
    case CPM_OPT_FUSED:
        if (value < 0 || value > 8) return fail(CPM_ERR_ARG, "fused hour %lld", (long long)value);
        c->zg.fused_ok = value != 0;
        c->zg.fused_auto = value == 5;                                            // 5: where it pays
        c->zg.fused_pf = value == 3 || value == 4;                                // 3, 4: placing first (k_grouped_hour_pf)
        c->zg.fused_day = value >= 6;                                             // 6 .. 9: all hours of a run in one launch (k_grouped_day)
        c->zg.day_mix = value == 8 ? 0 : 1;                                       // 8: its placing blocks in front of the sampler workgroups instead of among them
        c->zg.fused_spin = (value == 2 || value == 4 || value == 7) ? 0u : cpm::kFusedSpinLimit;  // 2, 4, 7: the waiting side gives up at once (tests of the bail-out)
        return CPM_OK;
    case CPM_OPT_FUSED_LAG:
        if (value < 1 || value > (1 << 20)) return fail(CPM_ERR_ARG, "fused lag %lld", (long long)value);
        c->zg.fused_lag = static_cast<int>(value);
        return CPM_OK;
    case CPM_OPT_ZONE_ORDER:
        if (value < 0 || value > 2) return fail(CPM_ERR_ARG, "zone order %lld (0 zone order, 1 largest-first, 2 largest-first on sparse row packs)", (long long)value);
        c->zg.use_perm = static_cast<int>(value);
        return CPM_OK;
    case CPM_OPT_SPARSE_UPLOAD:
        if (value != 0 && value != 1) return fail(CPM_ERR_ARG, "sparse upload %lld (0 dense row packs, 1 sparse where the table qualifies)", (long long)value);
        c->sparse_upload = value != 0;  // (read when a table is installed: the installed one stays as it is)
        return CPM_OK;
    case CPM_OPT_FLOWS_KEPT:
        if (value != 0 && value != 1) return fail(CPM_ERR_ARG, "flows form %lld (0 one launch per hour, 1 one launch over the kept runs of all hours)", (long long)value);
        c->zg.flows_kept = value != 0;
        return CPM_OK;
    case CPM_OPT_LAST_HOUR:
        if (value != 0 && value != 1) return fail(CPM_ERR_ARG, "last hour %lld (0 the plain sampler, 1 counts only)", (long long)value);
        c->zg.count_only = c->zb.count_only = value != 0;
        return CPM_OK;
    case CPM_OPT_NARROW_PACK:
        if (value != 0 && value != 1) return fail(CPM_ERR_ARG, "narrow pack %lld (0 wide row packs, 1 narrow where the rule allows)", (long long)value);
        c->narrow_opt = static_cast<int>(value);  // (read in front of every grouped step: the packs are built there when they are missing)
        return CPM_OK;
    case CPM_OPT_PROFILE_KERNEL:
        if (value < CPM_PROFILE_SAMPLER || value > CPM_PROFILE_UPLOAD) return fail(CPM_ERR_ARG, "profile kernel %lld", (long long)value);
        c->prof_what = static_cast<int>(value);
        return CPM_OK;
    case CPM_OPT_PROFILE:
        c->profile = value != 0;
        c->prof_stride = value > 1 ? static_cast<int>(value) : 1;
        c->prof_seen = 0;
        c->n_prof = 0;  // (re)start the record; hourly launches append until read or reset
        return CPM_OK;
    default:
        return fail(CPM_ERR_ARG, "unknown option %d", option);
    }
}

int32_t cpm_get_info(cpm_ctx *c, int32_t what, int64_t *value_out)
{
    if (!c || !value_out) return fail(CPM_ERR_ARG, "null argument");
    switch (what) {
    case CPM_INFO_KERNEL:
        *value_out = pick_kernel(c);
        return CPM_OK;
    case CPM_INFO_CAP_MULT:
        *value_out = c->zg.cap_mult;
        return CPM_OK;
    case CPM_INFO_PARTS:
        *value_out = c->zg.parts;
        return CPM_OK;
    case CPM_INFO_FUSED:
        *value_out = fused_form(c);
        return CPM_OK;
    case CPM_INFO_NARROW_TIES: {  // (a blocking read: the stream is drained, one word comes back from the device)
        uint32_t ties = 0;
        if (c->d_narrow_ties) {
            HIP_TRY(hipSetDevice(c->device));
            if (c->ivp_pending) {
                int32_t rc_ivp = finish_ivp(c);
                if (rc_ivp != CPM_OK) return rc_ivp;
            }
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipMemcpy(&ties, c->d_narrow_ties, sizeof(ties), hipMemcpyDeviceToHost));
        }
        *value_out = ties;
        return CPM_OK;
    }
    case CPM_INFO_SPARSE_TABLES:
        *value_out = c->sparse_tables ? cpm::pack_row_words(c->Zq, c->pk_G, 1) : 0;
        return CPM_OK;
    case CPM_INFO_FUSED_BAILOUTS:
        *value_out = c->fused_bailouts;
        return CPM_OK;
    case CPM_INFO_P_DENSE:
        *value_out = c->have_cdf && (c->sparse_tables ? c->p_dense_valid : c->d_p.get() != nullptr) ? 1 : 0;
        return CPM_OK;
    case CPM_INFO_DEST_TANGENT_DENSE:
        *value_out = c->tan_valid && c->d_tan ? 1 : 0;
        return CPM_OK;
    case CPM_INFO_DEST_TANGENT_COMPACT:
        *value_out = c->sdp_valid && c->d_sdp ? 1 : 0;
        return CPM_OK;
    case CPM_INFO_LAST_KERNEL:
    case CPM_INFO_LAST_FORM:
    case CPM_INFO_LAST_HOUR:
    case CPM_INFO_STEPS_REPEATED:
        if (c->ivp_pending) {  // a record of committed steps: an IVP still in flight is committed (or repeated) first
            HIP_TRY(hipSetDevice(c->device));
            int32_t rc_ivp = finish_ivp(c);
            if (rc_ivp != CPM_OK) return rc_ivp;
        }
        *value_out = what == CPM_INFO_LAST_KERNEL ? c->last_kernel : what == CPM_INFO_LAST_FORM ? c->last_form : what == CPM_INFO_LAST_HOUR ? c->last_hour : c->steps_repeated;
        return CPM_OK;
    case CPM_INFO_BATCH:
        *value_out = c->batch_B;
        return CPM_OK;
    case CPM_INFO_TRAVEL_TABLE:  // what ensure_travel_tables left for the resident datamatrix
        *value_out = !c->tt_valid ? 0 : c->tts_valid ? (c->tts_fixed ? 1 : 2) : 3;
        return CPM_OK;
    case CPM_INFO_LAST_BATCH_FLEETS:
    case CPM_INFO_NARROW_PACK:
    case CPM_INFO_CELL_APPLIED:
    case CPM_INFO_CELL_HEAVY:
    case CPM_INFO_CELL_LAST:
    case CPM_INFO_CELL_PLACE:
    case CPM_INFO_CELL_BATCH:
        if (c->ivp_pending) {
            HIP_TRY(hipSetDevice(c->device));
            int32_t rc_ivp = finish_ivp(c);
            if (rc_ivp != CPM_OK) return rc_ivp;
        }
        *value_out = what == CPM_INFO_LAST_BATCH_FLEETS ? c->last_batch_fleets
                     : what == CPM_INFO_NARROW_PACK     ? (c->last_cells.narrow ? 1 : 0)
                     : what == CPM_INFO_CELL_APPLIED    ? c->last_cells.applied
                     : what == CPM_INFO_CELL_HEAVY      ? c->last_cells.heavy
                     : what == CPM_INFO_CELL_LAST       ? c->last_cells.last
                     : what == CPM_INFO_CELL_PLACE      ? c->last_cells.place
                                                        : c->last_cells.batch;
        return CPM_OK;
    default:
        return fail(CPM_ERR_ARG, "unknown info %d", what);
    }
}

int32_t cpm_set_stream(cpm_ctx *c, void *hip_stream)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (c->have_stream) {  // whatever was enqueued so far is finished on the stream it was enqueued on
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->stream = static_cast<hipStream_t>(hip_stream);
    c->have_stream = hip_stream != nullptr;  // NULL: the context's own stream, created when it is first needed
    return CPM_OK;
}

int32_t cpm_sync(cpm_ctx *c)
{
    CTX_TRY(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ tables

int32_t cpm_set_p_drive(cpm_ctx *c, const double *p_drive)
{
    CTX_TRY(c);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!p_drive) return fail(CPM_ERR_ARG, "null p_drive");
    size_t bytes = sizeof(double) * c->Z * c->T;
    if (!c->d_pdrive) HIP_TRY(hipMalloc(&c->d_pdrive, bytes));
    HIP_TRY(hipMemcpyAsync(c->d_pdrive, p_drive, bytes, hipMemcpyHostToDevice, c->stream));
    {
        int32_t rc_thr = update_thr(c);
        if (rc_thr != CPM_OK) return rc_thr;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_pdrive = true;
    return CPM_OK;
}

int32_t cpm_set_p_dest(cpm_ctx *c, const double *p_dest)
{
    CTX_TRY(c);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!p_dest) return fail(CPM_ERR_ARG, "null p_dest");
    size_t bytes = sizeof(double) * c->Z * c->Z * c->T;
    HIP_TRY(c->d_p.reserve(bytes / sizeof(double)));
    c->have_cdf = false;
    drop_dest_tangent(c);
    HIP_TRY(hipMemcpyAsync(c->d_p, p_dest, bytes, hipMemcpyHostToDevice, c->stream));
    if (c->sparse_upload) {  // sparse row packs where the table qualifies (cpm_upload.h)
        bool done = false;
        int32_t rc_sp = upload_p_dest_sparse(c, &done);
        if (rc_sp != CPM_OK || done) return rc_sp;
    }
    return build_rows(c, false);  // (synchronises: the validation flag is read back)
}

int32_t cpm_set_datamatrix(cpm_ctx *c, const double *datamatrix, const double *dist)
{
    CTX_TRY(c);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!datamatrix) return fail(CPM_ERR_ARG, "null datamatrix");
    size_t bytes = sizeof(double) * c->Z * c->Z * c->T * 2;
    size_t dbytes = sizeof(double) * c->Z * c->Z;
    HIP_TRY(c->d_dm.reserve(bytes / sizeof(double)));
    if (dist) HIP_TRY(c->d_dist.reserve(dbytes / sizeof(double)));
    c->have_dmat = false;
    c->tt_valid = false;
    c->tts_valid = false;
    c->ds_valid = false;
    drop_dest_tangent(c);
    c->pdrive_mean_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    HIP_TRY(hipMemcpyAsync(c->d_dm, datamatrix, bytes, hipMemcpyHostToDevice, c->stream));
    if (dist) HIP_TRY(hipMemcpyAsync(c->d_dist, dist, dbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_dmat = true;
    if (dist) c->have_dist = true;
    if (dist) c->dist_rows_valid = false;
    return CPM_OK;
}

// read_uber_csv with the C++ exceptions of its containers and threads turned into a message (nothing throws across the ABI)
static std::string read_csv_noexcept(const char *path, cpm::CsvRows &rows)
{
    try {
        const unsigned hw = std::thread::hardware_concurrency();
        return cpm::read_uber_csv(path, static_cast<int>(std::min(32u, hw ? hw : 4u)), rows, nullptr);
    } catch (const std::exception &e) {
        return std::string(path) + ": " + e.what();
    } catch (...) {
        return std::string(path) + ": unknown failure while reading";
    }
}

// createdatamatrix (src/createdatamatrix.jl:3-27) from rows already resident in d_raw (n x 5, column-major)
static int32_t datamatrix_from_device_rows(cpm_ctx *c, const double *d_raw, int64_t n)
{
    const size_t cells = static_cast<size_t>(c->Z) * c->Z * c->T;
    HIP_TRY(c->d_dm.reserve(cells * 2));
    c->have_dmat = false;
    c->tt_valid = false;
    c->tts_valid = false;
    c->ds_valid = false;
    drop_dest_tangent(c);
    c->pdrive_mean_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    HIP_TRY(hipMemsetAsync(c->d_dm, 0, sizeof(double) * cells * 2, c->stream));  // zeros(number_zones, number_zones, T, 2) (:7)
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->have_dmat = true;
        return CPM_OK;
    }
    DevBuf<uint32_t> d_owner;  // (scratch of this call: freed when it returns, behind the wait below)
    HIP_TRY(d_owner.reserve(cells));
    hipError_t e = hipMemsetAsync(d_owner, 0, sizeof(uint32_t) * cells, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cpm::k_dm_owner, dim3(nblk(n, 256)), dim3(256), 0, c->stream, d_raw, n, static_cast<int>(c->Z),
                           static_cast<int>(c->T), d_owner, c->d_err);
        hipLaunchKernelGGL(cpm::k_dm_write, dim3(nblk(n, 256)), dim3(256), 0, c->stream, d_raw, n, static_cast<int>(c->Z),
                           static_cast<int>(c->T), d_owner, c->d_dm);
        e = hipGetLastError();
    }
    int32_t rc = (e == hipSuccess) ? check_err_flag(c, "createdatamatrix: a row holds a zone id / hour that is not an integer in range "
                                                        "(reference: InexactError / BoundsError)", CPM_ERR_ARG)
                                   : fail(CPM_ERR_HIP, "createdatamatrix: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(c->stream);
    if (rc == CPM_OK) c->have_dmat = true;
    return rc;
}

int32_t cpm_parse_uber_csv(const char *path_to_csv_data, int64_t *n_rows_out, double *rawdata_out, int64_t capacity_rows)
{
    if (!path_to_csv_data || !n_rows_out) return fail(CPM_ERR_ARG, "parse_uber_csv: null argument");
    // the size query and the copy that follows it parse the file once: the rows of the last query are kept per thread
    thread_local cpm::CsvRows rows;
    thread_local std::string rows_key;
    struct stat st;
    if (stat(path_to_csv_data, &st) != 0) return fail(CPM_ERR_ARG, "parse_uber_csv: %s: %s", path_to_csv_data, strerror(errno));
    const std::string key = std::string(path_to_csv_data) + "|" + std::to_string(st.st_size) + "|" + std::to_string(st.st_mtim.tv_sec) +
                            "." + std::to_string(st.st_mtim.tv_nsec);
    if (key != rows_key) {
        rows_key.clear();
        std::string err = read_csv_noexcept(path_to_csv_data, rows);
        if (!err.empty()) return fail(CPM_ERR_ARG, "parse_uber_csv: %s", err.c_str());
        rows_key = key;
    }
    *n_rows_out = rows.n;
    if (!rawdata_out) return CPM_OK;
    rows_key.clear();  // handed over below: do not keep a second copy
    if (capacity_rows < rows.n) return fail(CPM_ERR_ARG, "parse_uber_csv: %lld rows, room for %lld", (long long)rows.n, (long long)capacity_rows);
    for (int k = 0; k < 5; ++k)
        std::memcpy(rawdata_out + static_cast<size_t>(k) * capacity_rows, rows.col[k].data(), sizeof(double) * static_cast<size_t>(rows.n));
    rows = cpm::CsvRows();
    return CPM_OK;
}

int32_t cpm_createdatamatrix_rows(cpm_ctx *c, int64_t n_rows, const double *rawdata)
{
    CTX_TRY(c);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (n_rows < 0 || n_rows >= (int64_t(1) << 32) - 1 || (n_rows > 0 && !rawdata)) return fail(CPM_ERR_ARG, "createdatamatrix: bad row list");
    DevBuf<double> d_raw;  // (scratch of this call; datamatrix_from_device_rows waits for the stream before it returns)
    if (n_rows > 0) {
        HIP_TRY(d_raw.reserve(5 * static_cast<size_t>(n_rows)));
        hipError_t e = hipMemcpyAsync(d_raw, rawdata, sizeof(double) * 5 * n_rows, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(CPM_ERR_HIP, "createdatamatrix: upload: %s", hipGetErrorString(e));
    }
    return datamatrix_from_device_rows(c, d_raw, n_rows);
}

int32_t cpm_createdatamatrix_csv(cpm_ctx *c, const char *path_to_csv_data, int64_t *n_rows_out)
{
    CTX_TRY(c);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!path_to_csv_data) return fail(CPM_ERR_ARG, "createdatamatrix: null path");
    cpm::CsvRows rows;
    std::string err = read_csv_noexcept(path_to_csv_data, rows);
    if (!err.empty()) return fail(CPM_ERR_ARG, "createdatamatrix: %s", err.c_str());
    if (n_rows_out) *n_rows_out = rows.n;
    if (rows.n >= (int64_t(1) << 32) - 1) return fail(CPM_ERR_ARG, "createdatamatrix: too many rows");
    DevBuf<double> d_raw;  // (scratch of this call; datamatrix_from_device_rows waits for the stream before it returns)
    if (rows.n > 0) {
        HIP_TRY(d_raw.reserve(5 * static_cast<size_t>(rows.n)));
        for (int k = 0; k < 5; ++k) {
            hipError_t e = hipMemcpyAsync(d_raw + static_cast<size_t>(k) * rows.n, rows.col[k].data(), sizeof(double) * rows.n,
                                          hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(c->stream);
                return fail(CPM_ERR_HIP, "createdatamatrix: upload: %s", hipGetErrorString(e));
            }
        }
    }
    return datamatrix_from_device_rows(c, d_raw, rows.n);
}

int32_t cpm_get_datamatrix(cpm_ctx *c, double *datamatrix_out)
{
    CTX_TRY(c);
    if (!datamatrix_out) return fail(CPM_ERR_ARG, "null out");
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "datamatrix not set");
    HIP_TRY(hipMemcpyAsync(datamatrix_out, c->d_dm, sizeof(double) * c->Z * c->Z * c->T * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_set_distance_from_centroids(cpm_ctx *c, const double *centroid_lat, const double *centroid_long)
{
    CTX_TRY(c);
    if (!centroid_lat || !centroid_long) return fail(CPM_ERR_ARG, "null centroids");
    const size_t dbytes = sizeof(double) * c->Z * c->Z;
    HIP_TRY(c->d_dist.reserve(dbytes / sizeof(double)));
    c->exp_trip_valid = c->exps_trip_valid = false;  // (before the first byte changes: a copy that fails half way leaves no weights behind)
    double *d_ll = nullptr;
    HIP_TRY(hipMalloc(&d_ll, sizeof(double) * 2 * c->Z));
    hipError_t e = hipMemcpyAsync(d_ll, centroid_lat, sizeof(double) * c->Z, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ll + c->Z, centroid_long, sizeof(double) * c->Z, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cpm::k_distance, dim3(nblk(c->Z, 256), static_cast<unsigned>(c->Z)), dim3(256), 0, c->stream, d_ll, d_ll + c->Z,
                           static_cast<int>(c->Z), c->d_dist);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dfree(d_ll);
    if (e != hipSuccess) return fail(CPM_ERR_HIP, "distance matrix: %s", hipGetErrorString(e));
    c->have_dist = true;
    c->dist_rows_valid = false;
    c->pdrive_mean_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    return CPM_OK;
}

int32_t cpm_set_distance(cpm_ctx *c, const double *dist)
{
    CTX_TRY(c);
    if (!dist) return fail(CPM_ERR_ARG, "null dist");
    const size_t dbytes = sizeof(double) * c->Z * c->Z;
    HIP_TRY(c->d_dist.reserve(dbytes / sizeof(double)));
    c->exp_trip_valid = c->exps_trip_valid = false;  // (before the first byte changes: a copy that fails half way leaves no weights behind)
    HIP_TRY(hipMemcpyAsync(c->d_dist, dist, dbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_dist = true;
    c->dist_rows_valid = false;
    c->pdrive_mean_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    return CPM_OK;
}

int32_t cpm_get_distance(cpm_ctx *c, double *dist_out)
{
    CTX_TRY(c);
    if (!dist_out) return fail(CPM_ERR_ARG, "null out");
    if (!c->have_dist) return fail(CPM_ERR_STATE, "distance matrix not set");
    HIP_TRY(hipMemcpyAsync(dist_out, c->d_dist, sizeof(double) * c->Z * c->Z, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_build_p_drive(cpm_ctx *c, double p_min, double p_max, double e_drive, double *out)
{
    CTX_TRY(c);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!c->have_dm()) return fail(CPM_ERR_STATE, "build_p_drive: datamatrix and distance matrix first (cpm_set_datamatrix, or cpm_createdatamatrix_* + cpm_set_distance_from_centroids)");
    size_t bytes = sizeof(double) * c->Z * c->T;
    if (!c->d_pdrive) HIP_TRY(hipMalloc(&c->d_pdrive, bytes));
    {
        int32_t rc_mean = ensure_pdrive_mean(c);
        if (rc_mean != CPM_OK) return rc_mean;
    }
    if (!c->d_thr) HIP_TRY(hipMalloc(&c->d_thr, sizeof(long long) * static_cast<size_t>(c->Z * c->T)));
    hipLaunchKernelGGL(cpm::k_pdrive_final, dim3(nblk(c->Z, 64), static_cast<unsigned>(c->T)), dim3(64), 0, c->stream, c->d_pdrive_mean,
                       c->d_pdrive, c->d_thr, static_cast<int>(c->Z), static_cast<int>(c->T), p_min, p_max, e_drive);  // (thresholds with it)
    hipError_t e = hipGetLastError();
    int32_t rc_thr = CPM_OK;
    if (e == hipSuccess && out) {  // (without a host copy to wait for the call returns as soon as the kernels are enqueued: everything that
        e = hipMemcpyAsync(out, c->d_pdrive, bytes, hipMemcpyDeviceToHost, c->stream);  // uses the table follows on the same stream)
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) return fail(CPM_ERR_HIP, "build_p_drive: %s", hipGetErrorString(e));
    if (rc_thr != CPM_OK) return rc_thr;
    c->have_pdrive = true;
    return CPM_OK;
}

static int32_t build_p_dest_tables(cpm_ctx *c, double e_dest, int32_t e_is_integer, double *out);

int32_t cpm_build_p_dest(cpm_ctx *c, double e_dest, int32_t e_is_integer, double *out)
{
    const int32_t rc = build_p_dest_tables(c, e_dest, e_is_integer, out);
    if (rc == CPM_OK) {  // what cpm_build_p_dest_tangent differentiates (include/cpm_expected_grad_dest.h)
        c->dest_built = true;
        c->dest_built_e = e_dest;
        c->dest_built_int = e_is_integer;
    }
    return rc;
}

static int32_t build_p_dest_tables(cpm_ctx *c, double e_dest, int32_t e_is_integer, double *out)
{
    CTX_TRY(c);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "build_p_dest: datamatrix first (cpm_set_datamatrix or cpm_createdatamatrix_*)");
    drop_dest_tangent(c);
    size_t bytes = sizeof(double) * c->Z * c->Z * c->T;
    {   // a sparse datamatrix: everything from its compact rows (cpm_dataset.h); p_destin itself only when the caller wants the array
        bool done = false;
        int32_t rc_sp = build_p_dest_sparse(c, e_dest, e_is_integer, &done);
        if (rc_sp != CPM_OK) return rc_sp;
        if (done) {
            if (!out) return CPM_OK;
            rc_sp = ensure_dense_p(c);
            if (rc_sp != CPM_OK) return rc_sp;
            HIP_TRY(hipMemcpyAsync(out, c->d_p, bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return CPM_OK;
        }
    }
    // createpdestin's array in the reference's layout: weights, then normalised in place.  It stays with the context (a sweep calls
    // this entry once per e_dest value: no allocation on that path); the row tables are derived from it in one more pass.
    HIP_TRY(c->d_p.reserve(bytes / sizeof(double)));
    c->have_cdf = false;
    dim3 g1(nblk(c->Z, 256), static_cast<unsigned>(c->Z));
    if (c->T == 24)
        hipLaunchKernelGGL(cpm::k_pdest_weights<24>, g1, dim3(256), 0, c->stream, c->d_dm, c->d_p, static_cast<int>(c->Z), static_cast<int>(c->T), e_dest, e_is_integer);
    else
        hipLaunchKernelGGL(cpm::k_pdest_weights<0>, g1, dim3(256), 0, c->stream, c->d_dm, c->d_p, static_cast<int>(c->Z), static_cast<int>(c->T), e_dest, e_is_integer);
    // (row sums into the row-total array, which the row builder overwrites behind them)
    if (!c->d_last) HIP_TRY(hipMalloc(&c->d_last, sizeof(double) * static_cast<size_t>(c->T * c->Z)));
    hipLaunchKernelGGL(cpm::k_pdest_rowsum, dim3(nblk(c->Z, 64), static_cast<unsigned>(c->T)), dim3(64), 0, c->stream, c->d_p, c->d_last, static_cast<int>(c->Z));
    hipLaunchKernelGGL(cpm::k_pdest_divide, dim3(nblk(c->Z, 256), nblk(c->Z, cpm::kDivBatch), static_cast<unsigned>(c->T)), dim3(256), 0, c->stream, c->d_p,
                       c->d_last, static_cast<int>(c->Z));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && out) e = hipMemcpyAsync(out, c->d_p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(CPM_ERR_HIP, "build_p_dest: %s", hipGetErrorString(e));
    return build_rows(c, false);  // (synchronises)
}

int32_t cpm_get_p_drive(cpm_ctx *c, double *out)
{
    CTX_TRY(c);
    if (!out) return fail(CPM_ERR_ARG, "null out");
    if (!c->have_pdrive) return fail(CPM_ERR_STATE, "p_drive not set");
    HIP_TRY(hipMemcpyAsync(out, c->d_pdrive, sizeof(double) * c->Z * c->T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_get_cdf_row(cpm_ctx *c, int64_t origin1, int64_t hour1, double *out)
{
    CTX_TRY(c);
    if (!out) return fail(CPM_ERR_ARG, "null out");
    if (!c->have_cdf) return fail(CPM_ERR_STATE, "p_dest not set");
    if (origin1 < 1 || origin1 > c->Z || hour1 < 1 || hour1 > c->T) return fail(CPM_ERR_ARG, "row index out of range");
    {
        int32_t rc_cdf = ensure_full_cdf(c);
        if (rc_cdf != CPM_OK) return rc_cdf;
    }
    const double *src = c->d_cdf + (static_cast<size_t>(hour1 - 1) * c->Z + (origin1 - 1)) * c->Zp;
    HIP_TRY(hipMemcpyAsync(out, src, sizeof(double) * c->Z, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_synth_tables(cpm_ctx *c, uint64_t table_seed) { return cpm_synth_tables_skewed(c, table_seed, 0); }

int32_t cpm_synth_tables_skewed(cpm_ctx *c, uint64_t table_seed, int64_t skew_q)
{
    CTX_TRY(c);
    if (skew_q < 0 || (skew_q > 0 && c->Z % 7919 == 0)) return fail(CPM_ERR_ARG, "synth_tables: skew %lld", (long long)skew_q);
    {   // a pending asynchronous IVP must be committed (or, after an overflow, repeated) on the tables it was enqueued with
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    size_t pd_bytes = sizeof(double) * c->Z * c->T;
    if (!c->d_pdrive) HIP_TRY(hipMalloc(&c->d_pdrive, pd_bytes));
    hipLaunchKernelGGL(cpm::k_synth_p_drive, dim3(nblk(c->Z * c->T, 256)), dim3(256), 0, c->stream, c->d_pdrive,
                       static_cast<int>(c->Z), static_cast<int>(c->T), table_seed);
    HIP_TRY(hipGetLastError());
    {
        int32_t rc_thr = update_thr(c);
        if (rc_thr != CPM_OK) return rc_thr;
    }
    c->have_pdrive = true;
    HIP_TRY(c->d_p.reserve(static_cast<size_t>(c->Z * c->Z * c->T)));
    c->have_cdf = false;
    drop_dest_tangent(c);
    dim3 grid(nblk(c->Z, 64), static_cast<unsigned>(c->T));
    hipLaunchKernelGGL(cpm::k_synth_p_dest, grid, dim3(64), 0, c->stream, c->d_p, static_cast<int>(c->Z), table_seed, skew_q);
    HIP_TRY(hipGetLastError());
    return build_rows(c, false);
}

int32_t cpm_synth_datamatrix(cpm_ctx *c, uint64_t table_seed, double density)
{
    CTX_TRY(c);
    {
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!(density >= 0.0 && density <= 1.0)) return fail(CPM_ERR_ARG, "synth_datamatrix: density %g", density);
    const size_t cells = static_cast<size_t>(c->Z) * c->Z * c->T;
    HIP_TRY(c->d_dm.reserve(cells * 2));
    HIP_TRY(c->d_dist.reserve(static_cast<size_t>(c->Z * c->Z)));
    c->have_dmat = c->have_dist = false;
    c->dist_rows_valid = false;
    c->tt_valid = false;
    c->tts_valid = false;
    c->ds_valid = false;
    drop_dest_tangent(c);
    c->pdrive_mean_valid = false;
    c->exp_trip_valid = c->exps_trip_valid = false;
    hipLaunchKernelGGL(cpm::k_synth_datamatrix, dim3(nblk(c->Z, 256), static_cast<unsigned>(c->Z), static_cast<unsigned>(c->T)), dim3(256), 0, c->stream,
                       c->d_dm, static_cast<int>(c->Z), static_cast<int>(c->T), table_seed, density);
    hipLaunchKernelGGL(cpm::k_synth_dist, dim3(nblk(c->Z, 256), static_cast<unsigned>(c->Z)), dim3(256), 0, c->stream, c->d_dist, static_cast<int>(c->Z),
                       table_seed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_dmat = c->have_dist = true;
    return CPM_OK;
}

int32_t cpm_refresh_tables(cpm_ctx *c, int32_t with_f64_cdf)
{
    CTX_TRY(c);
    {
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!c->have_cdf) return fail(CPM_ERR_STATE, "refresh_tables: p_dest not set");
    if (c->sparse_tables && c->tables_uploaded) {  // (an uploaded table's packs come from the cells the table owns: no dataset has a say)
        int32_t rc_up = pack_uploaded_rows(c, c->pk_Zc);
        if (rc_up != CPM_OK) return rc_up;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return with_f64_cdf ? ensure_full_cdf(c) : CPM_OK;
    }
    if (c->sparse_tables) {  // (the tables of a compact dataset: its rows are what they are rebuilt from)
        if (!c->ds_valid || !c->ds_ok) return fail(CPM_ERR_STATE, "refresh_tables: the datamatrix these tables were built from has been replaced");
        bool done = false;
        int32_t rc_sp = build_p_dest_sparse(c, c->tab_e_dest, c->tab_e_int, &done);
        if (rc_sp != CPM_OK || !done) return rc_sp != CPM_OK ? rc_sp : fail(CPM_ERR_STATE, "refresh_tables: compact rows no longer usable");
        return with_f64_cdf ? ensure_full_cdf(c) : CPM_OK;
    }
    if (!c->d_p) return fail(CPM_ERR_STATE, "refresh_tables: p_dest not set");
    return build_rows(c, with_f64_cdf != 0);
}

// ------------------------------------------------------------------ cars

int32_t cpm_init_states_strided(cpm_ctx *c, int64_t C_total, int64_t cars_per_zone, int64_t car_first, int64_t car_stride, int64_t car_count)
{
    CTX_TRY(c);
    if (c->ivp_pending) {  // the state is being replaced: the pending IVP's result is moot
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->ivp_pending = false;
    }
    if (C_total < 0 || cars_per_zone < 1 || car_first < 0 || car_count < 0 || car_stride < 1 || car_stride > 0x7fffffffLL ||
        (car_count > 0 && car_first + (car_count - 1) * car_stride >= C_total))
        return fail(CPM_ERR_ARG, "init_states: bad car set {%lld + k * %lld, k < %lld} of %lld", (long long)car_first, (long long)car_stride,
                    (long long)car_count, (long long)C_total);
    if (C_total > 0 && (C_total - 1) / cars_per_zone >= c->Z)
        return fail(CPM_ERR_ARG, "init_states: C = %lld cars at %lld per zone exceed %lld zones", (long long)C_total,
                    (long long)cars_per_zone, (long long)c->Z);
    if (car_count >= (int64_t(1) << 32)) return fail(CPM_ERR_ARG, "init_states: more than 2^32 cars in one context");
    int32_t rc = ensure_cars(c, car_count);
    if (rc != CPM_OK) return rc;
    c->C_total = C_total;
    c->cpz = cars_per_zone;
    c->cars = cpm::CarIndex{car_first, static_cast<uint32_t>(car_stride)};
    c->zx.buckets0_valid = false;
    c->zg.buckets0_valid = false;
    c->zb.buckets0_valid = false;
    if (car_count > 0) {
        hipLaunchKernelGGL(cpm::k_init_states, dim3(nblk(car_count, 256)), dim3(256), 0, c->stream, c->d_zone0, c->cars, car_count, cars_per_zone);
        HIP_TRY(hipGetLastError());
    }
    c->have_state = true;
    return CPM_OK;
}

int32_t cpm_init_states(cpm_ctx *c, int64_t C_total, int64_t cars_per_zone, int64_t car_begin, int64_t car_count)
{
    return cpm_init_states_strided(c, C_total, cars_per_zone, car_begin, 1, car_count);
}

int32_t cpm_set_state(cpm_ctx *c, const int64_t *zones)
{
    CTX_TRY(c);
    if (!c->have_state) return fail(CPM_ERR_STATE, "set_state: cpm_init_states first (defines the car range)");
    if (c->ivp_pending) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->ivp_pending = false;
    }
    c->zx.buckets0_valid = false;
    c->zg.buckets0_valid = false;
    c->zb.buckets0_valid = false;
    if (c->n == 0) return CPM_OK;
    if (!zones) return fail(CPM_ERR_ARG, "null zones");
    int64_t *d_z = nullptr;
    HIP_TRY(hipMalloc(&d_z, sizeof(int64_t) * c->n));
    hipError_t e = hipMemcpyAsync(d_z, zones, sizeof(int64_t) * c->n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cpm::k_zones_from_i64, dim3(nblk(c->n, 256)), dim3(256), 0, c->stream, c->d_zone0, d_z, c->n,
                           c->Z, c->d_err);
        e = hipGetLastError();
    }
    int32_t rc = (e == hipSuccess) ? check_err_flag(c, "set_state: zone id outside 1..number_zones", CPM_ERR_ARG)
                                   : fail(CPM_ERR_HIP, "set_state: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(c->stream);
    dfree(d_z);
    return rc;
}

int32_t cpm_get_state(cpm_ctx *c, int64_t *zones_out)
{
    CTX_TRY(c);
    if (!c->have_state) return fail(CPM_ERR_STATE, "get_state: no car state");
    {
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (c->n == 0) return CPM_OK;
    if (!zones_out) return fail(CPM_ERR_ARG, "null zones_out");
    int64_t *d_z = nullptr;
    HIP_TRY(hipMalloc(&d_z, sizeof(int64_t) * c->n));
    hipLaunchKernelGGL(cpm::k_zones_to_i64, dim3(nblk(c->n, 256)), dim3(256), 0, c->stream, d_z, c->d_zone0, c->n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(zones_out, d_z, sizeof(int64_t) * c->n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dfree(d_z);
    if (e != hipSuccess) return fail(CPM_ERR_HIP, "get_state: %s", hipGetErrorString(e));
    return CPM_OK;
}

int32_t cpm_solve_ivp_async(cpm_ctx *c, uint64_t seed)
{
    CTX_TRY(c);
    return ivp_enqueue(c, seed);
}

int32_t cpm_solve_ivp(cpm_ctx *c, uint64_t seed, int64_t *initial_state_out)
{
    CTX_TRY(c);
    int32_t rc = ivp_enqueue(c, seed);
    if (rc != CPM_OK) return rc;
    rc = finish_ivp(c);
    if (rc != CPM_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (initial_state_out) return cpm_get_state(c, initial_state_out);
    return CPM_OK;
}

int32_t cpm_resample_dev(cpm_ctx *c, uint64_t seed, uint32_t flags, void *d_counts)
{
    CTX_TRY(c);
    if (!d_counts) return fail(CPM_ERR_ARG, "null d_counts");
    return resample_enqueue(c, seed, flags, static_cast<int64_t *>(d_counts));
}

int32_t cpm_resample(cpm_ctx *c, uint64_t seed, uint32_t flags, int64_t *parking, int64_t *driving,
                     int64_t *sum_tt_q16, int64_t *state_out, double *trans_out)
{
    CTX_TRY(c);
    if (!parking || !driving) return fail(CPM_ERR_ARG, "null count outputs");
    bool compat = state_out || trans_out;
    BlockingCall call(c);
    if (call.rc != CPM_OK) return call.rc;
    if (compat) c->kernel = CPM_KERNEL_CAR;  // the per-hour records of every car are kept by this path
    int32_t rc = resample_blocking(c, seed, flags);
    if (rc != CPM_OK) return rc;
    copy_counts(c, parking, driving, sum_tt_q16);
    if (compat && c->n > 0) {
        // one hour column at a time: state[:,t] and trans[:,t,1..4] are contiguous runs of C values
        int64_t n = c->n;
        char *d_cols = nullptr;
        HIP_TRY(hipMalloc(&d_cols, static_cast<size_t>(n) * 8 * 5));
        int64_t *d_state = reinterpret_cast<int64_t *>(d_cols);
        double *d_f = reinterpret_cast<double *>(d_cols) + n;
        bool travel = (flags & CPM_FLAG_TRAVEL) != 0;
        hipError_t e = hipSuccess;
        for (int t = 0; t < c->T && e == hipSuccess; ++t) {
            const uint32_t *zsrc = (t == 0) ? c->d_zone0 : c->d_rec + static_cast<size_t>(t - 1) * n;
            hipLaunchKernelGGL(cpm::k_export_hour, dim3(nblk(n, 256)), dim3(256), 0, c->stream, zsrc,
                               c->d_rec + static_cast<size_t>(t) * n, n, c->cars, d_state, d_f, d_f + n, d_f + 2 * n,
                               d_f + 3 * n, travel ? c->d_dm.get() : nullptr, c->d_dist, static_cast<int>(c->Z),
                               static_cast<int>(c->T), t, static_cast<uint32_t>(c->T - 1 + t), seed);
            e = hipGetLastError();
            if (e == hipSuccess && state_out)
                e = hipMemcpyAsync(state_out + static_cast<size_t>(t) * n, d_state, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream);
            for (int k = 0; k < 4 && e == hipSuccess && trans_out; ++k)
                e = hipMemcpyAsync(trans_out + (static_cast<size_t>(k) * c->T + t) * n, d_f + static_cast<size_t>(k) * n,
                                   sizeof(double) * n, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
        dfree(d_cols);
        if (e != hipSuccess) return fail(CPM_ERR_HIP, "compat export: %s", hipGetErrorString(e));
    }
    return CPM_OK;
}

// ------------------------------------------------------------------ OD trip counts (include/cpm_flows.h)
int32_t cpm_resample_flows_dev(cpm_ctx *c, uint64_t seed, uint32_t flags, void *d_counts, void *d_flows)
{
    CTX_TRY(c);
    if (!d_counts) return fail(CPM_ERR_ARG, "null d_counts");
    if (!d_flows) return fail(CPM_ERR_ARG, "null d_flows");
    cpm::SideDest side;
    side.flows.dense = static_cast<int32_t *>(d_flows);
    return resample_enqueue(c, seed, flags, static_cast<int64_t *>(d_counts), side);
}

int32_t cpm_resample_flows(cpm_ctx *c, uint64_t seed, uint32_t flags, int64_t *parking, int64_t *driving, int64_t *sum_tt_q16, int32_t *flows_out)
{
    CTX_TRY(c);
    if (!parking || !driving) return fail(CPM_ERR_ARG, "null count outputs");
    if (!flows_out) return fail(CPM_ERR_ARG, "null flows_out");
    BlockingCall call(c);
    if (call.rc != CPM_OK) return call.rc;
    const size_t cells = static_cast<size_t>(c->T) * c->Z * c->Z;
    HIP_TRY(c->d_flows.reserve(cells));
    cpm::SideDest side;
    side.flows.dense = c->d_flows;
    int32_t rc = resample_blocking(c, seed, flags, side);
    if (rc != CPM_OK) return rc;
    copy_counts(c, parking, driving, sum_tt_q16);
    // (the flows of the attempt whose counts were fetched: every attempt writes the whole array, and the last one enqueued is the one returned)
    HIP_TRY(hipMemcpyAsync(flows_out, c->d_flows, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ parking stays (include/cpm_stays.h)
int32_t cpm_resample_stays_dev(cpm_ctx *c, uint64_t seed, uint32_t flags, void *d_counts, void *d_stays, void *d_parked)
{
    CTX_TRY(c);
    if (!d_counts) return fail(CPM_ERR_ARG, "null d_counts");
    if (!d_stays) return fail(CPM_ERR_ARG, "null d_stays");
    if (!d_parked) return fail(CPM_ERR_ARG, "null d_parked");
    cpm::SideDest side;
    side.stays.stays = static_cast<int32_t *>(d_stays);
    side.stays.parked = static_cast<int32_t *>(d_parked);
    return resample_enqueue(c, seed, flags, static_cast<int64_t *>(d_counts), side);
}

int32_t cpm_resample_stays(cpm_ctx *c, uint64_t seed, uint32_t flags, int64_t *parking, int64_t *driving, int64_t *sum_tt_q16, int32_t *stays_out,
                           int32_t *parked_out)
{
    CTX_TRY(c);
    if (!parking || !driving) return fail(CPM_ERR_ARG, "null count outputs");
    if (!stays_out) return fail(CPM_ERR_ARG, "null stays_out");
    if (!parked_out) return fail(CPM_ERR_ARG, "null parked_out");
    BlockingCall call(c);
    if (call.rc != CPM_OK) return call.rc;
    const size_t zt = static_cast<size_t>(c->Z * c->T), cells = zt * static_cast<size_t>(c->T);
    HIP_TRY(c->d_stays.reserve(cells));
    HIP_TRY(c->d_stay_parked.reserve(zt));
    cpm::SideDest side;
    side.stays.stays = c->d_stays;
    side.stays.parked = c->d_stay_parked;
    int32_t rc = resample_blocking(c, seed, flags, side);
    if (rc != CPM_OK) return rc;
    copy_counts(c, parking, driving, sum_tt_q16);
    // (the stays of the attempt whose counts were fetched: every attempt resets the side array and writes both arrays whole, and the
    //  last one enqueued is the one returned)
    HIP_TRY(hipMemcpyAsync(stays_out, c->d_stays, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(parked_out, c->d_stay_parked, sizeof(int32_t) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ charge (include/cpm_charge.h)
// the scalar parameters, checked, and the caller's arrays into a ChargeDest (the side array and the distance matrix: resample_enqueue)
static int32_t charge_dest(const cpm_charge_params *p, cpm::ChargeDest &cd)
{
    if (!p) return fail(CPM_ERR_ARG, "null params");
    if (p->capacity_wh < 1) return fail(CPM_ERR_ARG, "charge: capacity_wh = 0");
    if (p->initial_wh > p->capacity_wh) return fail(CPM_ERR_ARG, "charge: initial_wh = %u above capacity_wh = %u", p->initial_wh, p->capacity_wh);
    if (!(p->wh_per_km >= 0.0) || !(p->wh_per_km <= 1.7976931348623157e308)) return fail(CPM_ERR_ARG, "charge: wh_per_km = %g is not finite and >= 0", p->wh_per_km);
    cd.capacity = p->capacity_wh;
    cd.power = p->power_wh;
    cd.initial = p->initial_wh;
    cd.wh_per_km = p->wh_per_km;
    cd.zone_power = p->zone_power_wh;
    cd.soc_in = p->soc_in;
    return CPM_OK;
}

int32_t cpm_resample_charge_dev(cpm_ctx *c, uint64_t seed, uint32_t flags, const cpm_charge_params *params, void *d_counts, void *d_charge, void *d_used,
                                void *d_short, void *d_soc)
{
    CTX_TRY(c);
    if (!d_counts) return fail(CPM_ERR_ARG, "null d_counts");
    if (!d_charge) return fail(CPM_ERR_ARG, "null d_charge");
    if (!d_used) return fail(CPM_ERR_ARG, "null d_used");
    if (!d_short) return fail(CPM_ERR_ARG, "null d_short");
    cpm::SideDest side;
    int32_t rc = charge_dest(params, side.charge);
    if (rc != CPM_OK) return rc;
    side.charge.charge = static_cast<int64_t *>(d_charge);
    side.charge.used = static_cast<int64_t *>(d_used);
    side.charge.shrt = static_cast<int32_t *>(d_short);
    side.charge.soc = static_cast<uint32_t *>(d_soc);
    return resample_enqueue(c, seed, flags, static_cast<int64_t *>(d_counts), side);
}

int32_t cpm_resample_charge(cpm_ctx *c, uint64_t seed, uint32_t flags, const cpm_charge_params *params, int64_t *parking, int64_t *driving,
                            int64_t *sum_tt_q16, int64_t *charge_out, int64_t *used_out, int32_t *short_out, uint32_t *soc_out)
{
    CTX_TRY(c);
    if (!parking || !driving) return fail(CPM_ERR_ARG, "null count outputs");
    if (!charge_out) return fail(CPM_ERR_ARG, "null charge_out");
    if (!used_out) return fail(CPM_ERR_ARG, "null used_out");
    if (!short_out) return fail(CPM_ERR_ARG, "null short_out");
    cpm::SideDest side;
    cpm::ChargeDest &cd = side.charge;
    {
        int32_t rc_p = charge_dest(params, cd);
        if (rc_p != CPM_OK) return rc_p;
    }
    BlockingCall call(c);
    if (call.rc != CPM_OK) return call.rc;
    const size_t zt = static_cast<size_t>(c->Z * c->T), n = static_cast<size_t>(c->n);
    HIP_TRY(c->d_chg_load.reserve(2 * zt));
    HIP_TRY(c->d_chg_short.reserve(zt));
    HIP_TRY(c->d_chg_zone_power.reserve(static_cast<size_t>(c->Z)));
    const size_t soc_words = 2 * std::max<size_t>(n, 1);  // soc_in | soc_out: an even count, so that the halves of a grown array stay apart
    if (!c->d_chg_soc.fits(soc_words)) HIP_TRY(hipStreamSynchronize(c->stream));  // (a _dev step in flight may not read it, but nothing is freed under the stream)
    HIP_TRY(c->d_chg_soc.reserve(soc_words));
    // the caller's host arrays to the device (pageable memory: the copies have left the host when the calls return)
    if (cd.zone_power) {
        HIP_TRY(hipMemcpyAsync(c->d_chg_zone_power, cd.zone_power, sizeof(uint32_t) * c->Z, hipMemcpyHostToDevice, c->stream));
        cd.zone_power = c->d_chg_zone_power;
    }
    if (cd.soc_in) {
        if (n) HIP_TRY(hipMemcpyAsync(c->d_chg_soc, cd.soc_in, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
        cd.soc_in = c->d_chg_soc;
    }
    cd.charge = c->d_chg_load;
    cd.used = c->d_chg_load + zt;
    cd.shrt = c->d_chg_short;
    cd.soc = soc_out ? c->d_chg_soc + c->d_chg_soc.cap / 2 : nullptr;
    int32_t rc = resample_blocking(c, seed, flags, side);
    if (rc != CPM_OK) return rc;
    copy_counts(c, parking, driving, sum_tt_q16);
    // (the arrays of the attempt whose counts were fetched: every attempt fills the side array anew and writes every array whole, and
    //  the last one enqueued is the one returned)
    HIP_TRY(hipMemcpyAsync(charge_out, cd.charge, sizeof(int64_t) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(used_out, cd.used, sizeof(int64_t) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(short_out, cd.shrt, sizeof(int32_t) * zt, hipMemcpyDeviceToHost, c->stream));
    if (soc_out && n) HIP_TRY(hipMemcpyAsync(soc_out, cd.soc, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ per-car day records (include/cpm_paths.h)
int32_t cpm_resample_paths_dev(cpm_ctx *c, uint64_t seed, uint32_t flags, void *d_counts, void *d_paths)
{
    CTX_TRY(c);
    if (!d_counts) return fail(CPM_ERR_ARG, "null d_counts");
    if (!d_paths) return fail(CPM_ERR_ARG, "null d_paths");
    cpm::SideDest side;
    side.paths.paths = static_cast<uint32_t *>(d_paths);
    return resample_enqueue(c, seed, flags, static_cast<int64_t *>(d_counts), side);
}

int32_t cpm_resample_paths(cpm_ctx *c, uint64_t seed, uint32_t flags, int64_t *parking, int64_t *driving, int64_t *sum_tt_q16, uint32_t *paths_out)
{
    CTX_TRY(c);
    if (!parking || !driving) return fail(CPM_ERR_ARG, "null count outputs");
    if (!paths_out) return fail(CPM_ERR_ARG, "null paths_out");
    BlockingCall call(c);
    if (call.rc != CPM_OK) return call.rc;
    const int64_t words = c->T * c->n;
    HIP_TRY(c->d_paths.reserve(static_cast<size_t>(words)));  // kept from the first use (until the fleet grows)
    cpm::SideDest side;
    side.paths.paths = c->d_paths;
    int32_t rc = resample_blocking(c, seed, flags, side);
    if (rc != CPM_OK) return rc;
    copy_counts(c, parking, driving, sum_tt_q16);
    // (the record of the attempt whose counts were fetched: every attempt writes every word, and the last one enqueued is the one returned)
    if (words > 0) {
        HIP_TRY(hipMemcpyAsync(paths_out, c->d_paths, sizeof(uint32_t) * static_cast<size_t>(words), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CPM_OK;
}

// k_export_hour as cpm_resample's compat route launches it, with the record in the place of the per-car kernels' d_rec and the
// caller's device columns in the place of the staging columns: T launches on the stream, no synchronisation
int32_t cpm_paths_expand_dev(cpm_ctx *c, uint64_t seed, uint32_t flags, const void *d_paths, void *d_state, void *d_trans)
{
    CTX_TRY(c);
    if (!d_paths) return fail(CPM_ERR_ARG, "null d_paths");
    {
        int32_t rc_ivp = finish_ivp(c);
        if (rc_ivp != CPM_OK) return rc_ivp;
    }
    if (!c->have_state) return fail(CPM_ERR_STATE, "paths_expand: no car state (cpm_init_states / cpm_set_state)");
    const bool travel = (flags & CPM_FLAG_TRAVEL) != 0;
    if (travel && !c->have_dm()) return fail(CPM_ERR_STATE, "CPM_FLAG_TRAVEL needs cpm_set_datamatrix");
    const int64_t n = c->n;
    if (n == 0 || (!d_state && !d_trans)) return CPM_OK;
    int64_t *spare_state = nullptr;
    double *spare_f = nullptr;
    if (!d_state || !d_trans) {  // (the kernel writes all five columns: those nobody asked for go to the context's own)
        HIP_TRY(c->d_expand_cols.reserve(static_cast<size_t>(n) * 8 * 5));
        spare_state = reinterpret_cast<int64_t *>(c->d_expand_cols.get());
        spare_f = reinterpret_cast<double *>(c->d_expand_cols.get()) + n;
    }
    const uint32_t *rec = static_cast<const uint32_t *>(d_paths);
    const size_t tn = static_cast<size_t>(c->T) * n;
    for (int t = 0; t < c->T; ++t) {
        const uint32_t *zsrc = (t == 0) ? c->d_zone0 : rec + static_cast<size_t>(t - 1) * n;
        int64_t *state_col = d_state ? static_cast<int64_t *>(d_state) + static_cast<size_t>(t) * n : spare_state;
        double *f = d_trans ? static_cast<double *>(d_trans) + static_cast<size_t>(t) * n : spare_f;
        const size_t col = d_trans ? tn : static_cast<size_t>(n);
        hipLaunchKernelGGL(cpm::k_export_hour, dim3(nblk(n, 256)), dim3(256), 0, c->stream, zsrc, rec + static_cast<size_t>(t) * n, n, c->cars, state_col, f,
                           f + col, f + 2 * col, f + 3 * col, travel ? c->d_dm.get() : nullptr, c->d_dist, static_cast<int>(c->Z), static_cast<int>(c->T), t,
                           static_cast<uint32_t>(c->T - 1 + t), seed);
        HIP_TRY(hipGetLastError());
    }
    return CPM_OK;
}

// ------------------------------------------------------------------ OD trip counts as compressed sparse rows (include/cpm_flows_csr.h)
int32_t cpm_resample_flows_csr_dev(cpm_ctx *c, uint64_t seed, uint32_t flags, void *d_counts, void *d_row_ptr, void *d_dest, void *d_count, int64_t cap)
{
    CTX_TRY(c);
    if (!d_counts) return fail(CPM_ERR_ARG, "null d_counts");
    if (!d_row_ptr) return fail(CPM_ERR_ARG, "null d_row_ptr");
    if (cap < 0) return fail(CPM_ERR_ARG, "negative cap");
    if (cap > 0 && (!d_dest || !d_count)) return fail(CPM_ERR_ARG, "null d_dest / d_count with cap > 0");
    cpm::SideDest side;
    side.flows.row_ptr = static_cast<int64_t *>(d_row_ptr);
    side.flows.dest = static_cast<int32_t *>(d_dest);
    side.flows.count = static_cast<int32_t *>(d_count);
    side.flows.cap = cap;
    return resample_enqueue(c, seed, flags, static_cast<int64_t *>(d_counts), side);
}

int32_t cpm_resample_flows_csr(cpm_ctx *c, uint64_t seed, uint32_t flags, int64_t *parking, int64_t *driving, int64_t *sum_tt_q16, int64_t *row_ptr_out,
                               int64_t *nnz_out)
{
    CTX_TRY(c);
    if (!parking || !driving) return fail(CPM_ERR_ARG, "null count outputs");
    if (!row_ptr_out || !nnz_out) return fail(CPM_ERR_ARG, "null row_ptr_out / nnz_out");
    BlockingCall call(c);
    if (call.rc != CPM_OK) return call.rc;
    c->csr_nnz = -1;
    const size_t zt = static_cast<size_t>(c->Z * c->T);
    HIP_TRY(c->d_csr_row_ptr.reserve(zt + 1));
    // T * min(n, Z * Z) entries always suffice.  The arrays start at that bound, or at 1 GiB for the two where the bound is larger;
    // a step that needs more tells by row_ptr[T * Z], which is exact whatever the capacity, and is run again on arrays of that size.
    auto csr_cap = [&] { return static_cast<int64_t>(c->d_csr_count.cap); };  // (both arrays: grown together, the second one last)
    auto ensure_entries = [&](int64_t want) -> int32_t {
        HIP_TRY(c->d_csr_dest.reserve(static_cast<size_t>(want)));
        HIP_TRY(c->d_csr_count.reserve(static_cast<size_t>(want)));
        return CPM_OK;
    };
    const int64_t bound = static_cast<int64_t>(c->T) * std::min<int64_t>(c->n, static_cast<int64_t>(c->Z) * c->Z);
    int32_t rc = ensure_entries(std::max<int64_t>(std::min<int64_t>(bound, (int64_t{1} << 30) / 8), 1));
    if (rc != CPM_OK) return rc;
    for (int attempt = 0;; ++attempt) {
        cpm::SideDest side;
        side.flows.row_ptr = c->d_csr_row_ptr;
        side.flows.dest = c->d_csr_dest;
        side.flows.count = c->d_csr_count;
        side.flows.cap = csr_cap();
        rc = resample_blocking(c, seed, flags, side);
        if (rc != CPM_OK) return rc;
        // (the rows of the attempt whose counts were fetched: every attempt writes all of row_ptr, and the last one enqueued is the one returned)
        HIP_TRY(hipMemcpyAsync(row_ptr_out, c->d_csr_row_ptr, sizeof(int64_t) * (zt + 1), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int64_t nnz = row_ptr_out[zt];
        if (nnz < 0 || nnz > bound) return fail(CPM_ERR_HIP, "flows (csr): %lld entries reported, at most %lld possible", (long long)nnz, (long long)bound);
        if (nnz <= csr_cap()) break;
        if (attempt > 0) return fail(CPM_ERR_HIP, "flows (csr): %lld entries after a run that reported fewer", (long long)nnz);
        rc = ensure_entries(nnz);  // (the step is a pure function of seed and state: the repeat needs exactly as many)
        if (rc != CPM_OK) return rc;
    }
    copy_counts(c, parking, driving, sum_tt_q16);
    c->csr_nnz = row_ptr_out[zt];
    *nnz_out = c->csr_nnz;
    return CPM_OK;
}

int32_t cpm_get_flows_csr(cpm_ctx *c, int32_t *dest_out, int32_t *count_out, int64_t nnz)
{
    CTX_TRY(c);
    if (c->csr_nnz < 0) return fail(CPM_ERR_ARG, "cpm_get_flows_csr: no cpm_resample_flows_csr before it");
    if (nnz != c->csr_nnz) return fail(CPM_ERR_ARG, "cpm_get_flows_csr: nnz %lld, the last cpm_resample_flows_csr reported %lld", (long long)nnz, (long long)c->csr_nnz);
    if (nnz > 0 && (!dest_out || !count_out)) return fail(CPM_ERR_ARG, "null dest_out / count_out");
    if (nnz == 0) return CPM_OK;
    HIP_TRY(hipMemcpyAsync(dest_out, c->d_csr_dest, sizeof(int32_t) * static_cast<size_t>(nnz), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(count_out, c->d_csr_count, sizeof(int32_t) * static_cast<size_t>(nnz), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_last_kernel_ms(cpm_ctx *c, float *ms_out, int32_t cap, int32_t *n_out)
{
    CTX_TRY(c);
    if (!ms_out || !n_out) return fail(CPM_ERR_ARG, "null output");
    HIP_TRY(hipStreamSynchronize(c->stream));
    int n = std::min<int>(c->n_prof, cap);
    for (int k = 0; k < n; ++k) HIP_TRY(hipEventElapsedTime(&ms_out[k], c->ev[2 * k], c->ev[2 * k + 1]));
    *n_out = n;
    return CPM_OK;
}

int32_t cpm_algorithmic_bytes_per_hour(cpm_ctx *c, int64_t *bytes_out)
{
    if (!c || !bytes_out) return fail(CPM_ERR_ARG, "null argument");
    // B/T = Z*Z*8 (CDF slab) + Z*8 (p_drive) + C_g*8 (4 B zone in + 4 B out) + 2*Z*8 (counts)
    // The second-generation grouped path streams the 4-byte high-word rows (Zq per row) instead of the f64 rows:
    // its true element size is substituted, as 8(d) prescribes for a variant with a different element size.
    const bool hi_rows = pick_kernel(c) == CPM_KERNEL_ZONE_GROUPED && grouped_fits(c, c->zg.cap_mult);
    // ... and where the one-launch hour streams NARROW packs (cpm_narrow.h), theirs.
    const int64_t pack_words = hi_rows && narrow_wanted(c) ? cpm::narrow_row_words(c->Zq, c->pk_G) : cpm::pack_row_words(c->Zq, c->pk_G, c->sparse_tables);
    const int64_t rows = hi_rows ? c->Z * pack_words * 4 + c->Z * 8
                                 : c->Z * c->Z * 8;
    *bytes_out = rows + c->Z * 8 + c->n * 8 + 2 * c->Z * 8;
    return CPM_OK;
}

int32_t cpm_debug_categorical(cpm_ctx *c, int64_t origin1, int64_t hour1, int64_t n, const uint64_t *k53, int64_t *dest_out,
                              int32_t *n_exact_out)
{
    CTX_TRY(c);
    if (!c->have_cdf || !c->d_hi) return fail(CPM_ERR_STATE, "debug_categorical: p_dest not set (or rows too long for the high-word table)");
    if (origin1 < 1 || origin1 > c->Z || hour1 < 1 || hour1 > c->T) return fail(CPM_ERR_ARG, "row index out of range");
    if (n < 0 || (n > 0 && (!k53 || !dest_out))) return fail(CPM_ERR_ARG, "bad draw list");
    if (n_exact_out) *n_exact_out = 0;
    if (n == 0) return CPM_OK;
    const size_t row = static_cast<size_t>(hour1 - 1) * c->Z + (origin1 - 1);
    uint64_t *d_k = nullptr;
    int64_t *d_o = nullptr;
    int *d_n = nullptr;
    hipError_t e = hipMalloc(&d_k, sizeof(uint64_t) * n);
    if (e == hipSuccess) e = hipMalloc(&d_o, sizeof(int64_t) * n);
    if (e == hipSuccess) e = hipMalloc(&d_n, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(d_n, 0, sizeof(int), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_k, k53, sizeof(uint64_t) * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const int G = c->pk_G;
        const size_t words = static_cast<size_t>(cpm::pack_row_words(c->Zq, G, c->sparse_tables));
        const size_t lds = sizeof(uint32_t) * words;
        e = cpm::lds_opt_in<cpm::k_pack_search_debug>(lds, cpm::kPackLds);
        const size_t th = static_cast<size_t>(hour1 - 1);
        uint32_t h_scnt = 0;
        if (e == hipSuccess && c->sparse_tables) {
            e = hipMemcpyAsync(&h_scnt, c->d_scnt + row, sizeof h_scnt, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
        if (e == hipSuccess) {
            const bool sp = c->sparse_tables;
            hipLaunchKernelGGL(cpm::k_pack_search_debug, dim3(1), dim3(512), lds, c->stream, c->d_hi + row * words, c->d_last + row,
                               sp ? nullptr : c->d_ckpt + th * cpm::ckpt_count(static_cast<int>(c->Z)) * c->Z, sp ? nullptr : c->d_p + th * c->Z * c->Z,
                               static_cast<int>(origin1 - 1), static_cast<int>(c->Z), c->Zq, G, c->pk_Zc, sp ? c->d_sp + row * cpm::kDsCap : nullptr,
                               sp ? c->d_sj + row * cpm::kDsCap : nullptr, std::min(h_scnt, cpm::kDsCap), n, d_k, d_o, d_n);
            e = hipGetLastError();
        }
    }
    int h_n = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(dest_out, d_o, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_n, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dfree(d_k);
    dfree(d_o);
    dfree(d_n);
    if (e != hipSuccess) return fail(CPM_ERR_HIP, "debug_categorical: %s", hipGetErrorString(e));
    if (n_exact_out) *n_exact_out = h_n;
    return CPM_OK;
}

int32_t cpm_debug_travel_draw(cpm_ctx *c, int64_t n, const uint64_t *k53, const double *mean, const double *sd, double *draw_out,
                              double *mass_out, int64_t *q16_out)
{
    CTX_TRY(c);
    if (n < 0 || (n > 0 && (!k53 || !mean || !sd || !draw_out || !mass_out || !q16_out))) return fail(CPM_ERR_ARG, "debug_travel_draw: bad argument list");
    if (n == 0) return CPM_OK;
    const size_t bytes = sizeof(double) * static_cast<size_t>(n);  // (every array holds n 8-byte elements)
    char *d = nullptr;                                              // k53 | mean | sd | draw | mass | q16
    hipError_t e = hipMalloc(&d, 6 * bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d, k53, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + bytes, mean, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + 2 * bytes, sd, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cpm::k_debug_travel_draw, dim3(nblk(n, 256)), dim3(256), 0, c->stream, n, reinterpret_cast<const uint64_t *>(d),
                           reinterpret_cast<const double *>(d + bytes), reinterpret_cast<const double *>(d + 2 * bytes),
                           reinterpret_cast<double *>(d + 3 * bytes), reinterpret_cast<double *>(d + 4 * bytes),
                           reinterpret_cast<long long *>(d + 5 * bytes));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(draw_out, d + 3 * bytes, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(mass_out, d + 4 * bytes, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q16_out, d + 5 * bytes, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dfree(d);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CPM_ERR_NOMEM : CPM_ERR_HIP, "debug_travel_draw: %s", hipGetErrorString(e));
    return CPM_OK;
}

int32_t cpm_debug_f64_kit(cpm_ctx *c, int32_t fn, int64_t n, const double *x, double *out)
{
    CTX_TRY(c);
    if (fn < CPM_KIT_LOG || fn > CPM_KIT_EXP_NEG) return fail(CPM_ERR_ARG, "debug_f64_kit: unknown function %d", fn);
    if (n < 0 || (n > 0 && (!x || !out))) return fail(CPM_ERR_ARG, "debug_f64_kit: bad argument list");
    if (n == 0) return CPM_OK;
    const size_t bytes = sizeof(double) * static_cast<size_t>(n);
    char *d = nullptr;  // x | out
    hipError_t e = hipMalloc(&d, 2 * bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d, x, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cpm::k_debug_f64_kit, dim3(nblk(n, 256)), dim3(256), 0, c->stream, static_cast<int>(fn), n,
                           reinterpret_cast<const double *>(d), reinterpret_cast<double *>(d + bytes));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + bytes, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dfree(d);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CPM_ERR_NOMEM : CPM_ERR_HIP, "debug_f64_kit: %s", hipGetErrorString(e));
    return CPM_OK;
}

// ------------------------------------------------------------------ the sweep's objectives (include/cpm_objectives.h)

int32_t cpm_set_measured(cpm_ctx *c, const double *measured)
{
    CTX_TRY(c);
    if (!measured) {  // (host state only: what is in flight on the stream was enqueued with the data it had)
        c->have_measured = false;
        return CPM_OK;
    }
    const size_t cells = static_cast<size_t>(c->Z) * static_cast<size_t>(c->T);
    for (size_t i = 0; i < cells; ++i)
        if (!std::isfinite(measured[i]))
            return fail(CPM_ERR_ARG, "set_measured: entry (zone %lld, hour %lld) is not finite", (long long)(i % c->Z) + 1, (long long)(i / c->Z) + 1);
    HIP_TRY(c->d_measured.reserve(cells));
    HIP_TRY(c->d_meas_flag.reserve(static_cast<size_t>(c->Z)));
    // (Z x T column-major IS [T][Z]: the layout the kernels read, Z contiguous like the count tensor)
    HIP_TRY(hipMemcpyAsync(c->d_measured, measured, sizeof(double) * cells, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cpm::k_measured_flag, dim3(nblk(c->Z, cpm::kObjBlock)), dim3(cpm::kObjBlock), 0, c->stream, c->d_measured, c->d_meas_flag,
                       static_cast<int>(c->Z), static_cast<int>(c->T));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_measured = true;
    return CPM_OK;
}

int32_t cpm_objectives_dev(cpm_ctx *c, const void *d_counts, int32_t B, int64_t n_cars, void *d_obj, void *d_zone_err)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");
    if (!d_counts) return fail(CPM_ERR_ARG, "objectives: null d_counts");
    if (!d_obj) return fail(CPM_ERR_ARG, "objectives: null d_obj");
    if (B < 1 || B > CPM_MAX_BATCH) return fail(CPM_ERR_ARG, "objectives: B = %d outside 1..%d", B, CPM_MAX_BATCH);
    if (n_cars < 1) return fail(CPM_ERR_ARG, "objectives: n_cars = %lld", (long long)n_cars);
    CTX_TRY(c);
    const unsigned nb = nblk(c->Z, cpm::kObjBlock);
    HIP_TRY(c->d_obj_part.reserve(nb * static_cast<size_t>(B)));  // (a grow frees first: hipFree waits for what still reads the old workspace)
    HIP_TRY(c->d_obj_part_n.reserve(nb * static_cast<size_t>(B)));
    const int T = static_cast<int>(c->T);
    unsigned long long *obj = static_cast<unsigned long long *>(d_obj);
    // the hour sums are accumulated with atomics: the records start from zero
    HIP_TRY(hipMemsetAsync(obj, 0, sizeof(unsigned long long) * static_cast<size_t>(B) * static_cast<size_t>(cpm::kObjHead + 2 * T), c->stream));
    hipLaunchKernelGGL(cpm::k_obj_zones, dim3(nb, static_cast<unsigned>(B)), dim3(cpm::kObjBlock), 0, c->stream, static_cast<const long long *>(d_counts),
                       c->have_measured ? c->d_measured.get() : nullptr, c->have_measured ? c->d_meas_flag.get() : nullptr, static_cast<long long>(n_cars),
                       static_cast<int>(c->Z), T, obj, static_cast<double *>(d_zone_err), c->d_obj_part, c->d_obj_part_n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cpm::k_obj_final, dim3(static_cast<unsigned>(B)), dim3(64), 0, c->stream, static_cast<const long long *>(d_counts), c->d_obj_part,
                       c->d_obj_part_n, static_cast<int>(nb), static_cast<int>(c->Z), T, obj);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

// ------------------------------------------------------------------ expected densities (include/cpm_expected.h)

int32_t cpm_expected_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, void *d_out, void *d_pi_next)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_out) return fail(CPM_ERR_ARG, "expected_dev: null d_out");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<double *>(d_out),
                            static_cast<double *>(d_pi_next));
}

int32_t cpm_expected_batch_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, void *d_out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_out) return fail(CPM_ERR_ARG, "expected_batch_dev: null d_out");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    return expected_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<double *>(d_out), nullptr);
}

int32_t cpm_expected(cpm_ctx *c, const double *pi0, uint32_t flags, double *parking, double *driving, double *pi_next)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!parking || !driving) return fail(CPM_ERR_ARG, "expected: null density outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, parking, driving, pi_next);
}

int32_t cpm_expected_batch(cpm_ctx *c, const double *pi0, uint32_t flags, double *parking, double *driving)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!parking || !driving) return fail(CPM_ERR_ARG, "expected_batch: null density outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    return expected_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, parking, driving, nullptr);
}

// ------------------------------------------------------------------ exact variances of the counts (include/cpm_expected_var.h)

namespace {

// a workspace of the variance call: a failed allocation names the bytes asked for
int32_t var_reserve(DevBuf<double> &b, size_t words, const char *what)
{
    if (b.reserve(words) == hipSuccess) return CPM_OK;
    (void)hipGetLastError();
    return fail(CPM_ERR_NOMEM, "expected_var: cannot allocate %s: %zu bytes asked for", what, words * sizeof(double));
}

// P_t through the day (and, with the IVP, through hours 0 .. T-2 in front of it) and the four weighted column sums of every hour:
// enqueued on the context's stream.  out: [4][T][Z].
int32_t expected_var_enqueue(cpm_ctx *c, const double *d_start, uint32_t flags, double *out)
{
    int32_t rc = exp_tables_ready(c, "expected_var");
    if (rc != CPM_OK) return rc;
    if ((rc = ensure_exp_aux(c)) != CPM_OK) return rc;  // (expands sparse tables to the dense array; the row-total check)
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t zz = static_cast<size_t>(Z) * Z;
    const int chunks = static_cast<int>(nblk(Z, cpm::kVarRedRows));
    if ((rc = var_reserve(c->d_var_p, 2 * zz, "the two transition matrices")) != CPM_OK) return rc;
    if ((rc = var_reserve(c->d_var_part, static_cast<size_t>(chunks) * 4 * Z, "the partial sums")) != CPM_OK) return rc;
    double *const pm[2] = {c->d_var_p, c->d_var_p + c->d_var_p.cap / 2};
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0;  // operators in front of the day
    const dim3 block(cpm::kVarBlock);
    const dim3 ggrid(nblk(Z, cpm::kVarTile), nblk(Z, cpm::kVarTile));
    auto sums = [&](const double *P, int t) {
        cpm::launch(cpm::k_var_reduce, dim3(nblk(Z, cpm::kVarBlock), static_cast<unsigned>(chunks)), block, 0, c->stream, P, d_start,
                    static_cast<const double *>(c->d_pdrive) + static_cast<size_t>(t) * Z, Z, c->d_var_part.get());
        cpm::launch(cpm::k_var_final, dim3(nblk(Z, cpm::kVarBlock), 4), block, 0, c->stream, static_cast<const double *>(c->d_var_part.get()), chunks, Z, T, t,
                    out);
    };
    cpm::launch(cpm::k_var_eye, dim3(nblk(static_cast<int64_t>(zz), cpm::kVarBlock)), block, 0, c->stream, pm[0], Z);
    HIP_TRY(hipGetLastError());
    if (pre == 0) sums(pm[0], 0);
    // step s applies the operator of hour (s < pre ? s : s - pre); the matrix behind step pre - 1 (or I) is hour 0 of the outputs
    const int steps = pre + T - 1;
    for (int s = 0; s < steps; ++s) {
        const int t = s < pre ? s : s - pre;
        const size_t row = static_cast<size_t>(t) * Z;
        const int in = s & 1, ot = in ^ 1;
        cpm::launch(cpm::k_var_gemm, ggrid, block, 0, c->stream, static_cast<const double *>(pm[in]), static_cast<const double *>(c->d_p + row * Z),
                    static_cast<const double *>(c->d_last + row), static_cast<const double *>(c->d_exp_r + row),
                    static_cast<const int *>(c->d_exp_ell + row), static_cast<const double *>(c->d_pdrive) + row, pm[ot], Z);
        const int day_next = s + 1 - pre;  // the hour of the day whose matrix this step produces (< 0: still in front of it)
        if (day_next >= 0) sums(pm[ot], day_next);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

int32_t var_enter(cpm_ctx *c, uint32_t flags)
{
    int32_t rc = exp_flags_check(flags);
    if (rc != CPM_OK) return rc;
    CTX_TRY(c);
    if (!c->have_pdrive) return fail(CPM_ERR_STATE, "expected_var: p_drive not set");
    return CPM_OK;
}

}  // namespace

int32_t cpm_expected_var_dev(cpm_ctx *c, const void *d_start, uint32_t flags, void *d_out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_out) return fail(CPM_ERR_ARG, "expected_var_dev: null d_out");
    if ((rc = var_enter(c, flags)) != CPM_OK) return rc;
    return expected_var_enqueue(c, static_cast<const double *>(d_start), flags, static_cast<double *>(d_out));
}

int32_t cpm_expected_var(cpm_ctx *c, const double *start, uint32_t flags, double *mean_parking, double *mean_driving, double *var_parking,
                         double *var_driving)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if ((rc = var_enter(c, flags)) != CPM_OK) return rc;
    if (start)
        for (int64_t z = 0; z < c->Z; ++z)
            if (!std::isfinite(start[z]) || start[z] < 0.0)
                return fail(CPM_ERR_ARG, "expected_var: start of zone %lld is NaN, infinite or negative", (long long)z + 1);
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    if ((rc = var_reserve(c->d_var_out, 4 * zt + c->Z, "the outputs")) != CPM_OK) return rc;
    double *const d_w = c->d_var_out + 4 * zt;
    if (start) HIP_TRY(hipMemcpyAsync(d_w, start, sizeof(double) * c->Z, hipMemcpyHostToDevice, c->stream));
    if ((rc = expected_var_enqueue(c, start ? d_w : nullptr, flags, c->d_var_out)) != CPM_OK) return rc;
    double *const host[4] = {mean_parking, mean_driving, var_parking, var_driving};
    for (int k = 0; k < 4; ++k)
        if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], c->d_var_out + k * zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ the variance of linear functionals (include/cpm_expected_linear_var.h)

static int32_t exps_rows_ready(const cpm_ctx *c, const char *what);  // (below, with the sparse entries)

namespace {

int32_t elv_reserve(DevBuf<double> &b, size_t words, const char *what)
{
    if (b.reserve(words) == hipSuccess) return CPM_OK;
    (void)hipGetLastError();
    return fail(CPM_ERR_NOMEM, "expected_linear_var: cannot allocate %s: %zu bytes asked for", what, words * sizeof(double));
}

// one backward product of a pass: the smallest instantiation that holds it
void launch_elv_u(cpm_ctx *c, int NB, const double *p_t, const double *st, int Zs, int nseg, int seg_len, int nf, double *part)
{
    const int Z = static_cast<int>(c->Z);
    const dim3 grid(nblk(Z, cpm::kGradStrip), static_cast<unsigned>(nseg)), block(cpm::kExpBlock);
    const auto k = NB == 4 ? ((Z & 1) ? cpm::k_elv_u<4, true> : cpm::k_elv_u<4, false>)
                 : NB == 2 ? ((Z & 1) ? cpm::k_elv_u<2, true> : cpm::k_elv_u<2, false>)
                           : ((Z & 1) ? cpm::k_elv_u<1, true> : cpm::k_elv_u<1, false>);
    cpm::launch(k, grid, block, 0, c->stream, p_t, st, Z, Zs, seg_len, nf, part);
}

// ... from the compact rows of the hour whose first row is `row` (k_exps_elv_u<NB>; ensure_exps has run)
void launch_exps_elv_u(cpm_ctx *c, int NB, size_t row, const double *st, int Zs, int nseg, int seg_len, int nf, double *part)
{
    const int Z = static_cast<int>(c->Z);
    const auto k = NB == 4 ? cpm::k_exps_elv_u<4> : NB == 2 ? cpm::k_exps_elv_u<2> : cpm::k_exps_elv_u<1>;
    cpm::launch(k, dim3(static_cast<unsigned>(Z)), dim3(cpm::kExpsGradBlock), 0, c->stream, static_cast<const double *>(c->d_sp + row * cpm::kDsCap),
                static_cast<const uint32_t *>(c->d_sj + row * cpm::kDsCap), static_cast<const uint32_t *>(c->d_scnt + row), cpm::kDsCap, st, Z, Zs, seg_len, nseg,
                nf, part);
}

// The backward pass for K functionals, operator-major with the passes of at most kElvNB functionals inside an operator (the hour's
// block of p is read once per pass), then the weighted totals: enqueued on the context's stream.  coeff: [K][2][T][Z]; out: [K][2];
// zone: [K][2][Z] or nullptr.
// d_elv_ws, in vectors of Zs words: the state ping and pong, [K4][2] each (K4 = K rounded up to whole passes; a pass's state is
// [Zs][2][NB] at its first functional's place), the segments' sums [nseg][3][kElvNB], and [K][2][Z] words where zone is nullptr.
// sparse: the products read the compact rows (k_exps_elv_u, passes of kExpsElvNB) and the per-table arrays of ensure_exps; d_p is
// neither read nor built.
int32_t expected_linear_var_enqueue(cpm_ctx *c, const double *d_start, uint32_t flags, int K, const double *coeff, double *out, double *zone,
                                    bool sparse = false)
{
    int32_t rc = exp_tables_ready(c, "expected_linear_var");
    if (rc != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps(c) : ensure_exp_aux(c)) != CPM_OK) return rc;  // (dense: expands sparse tables to the dense array; the row-total check)
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const int Zs = (Z + 1) & ~1;
    const int nseg = cpm::grad_segments(Z), seg_len = cpm::grad_segment_len(Z, nseg);
    const int pass = sparse ? cpm::kExpsElvNB : cpm::kElvNB;
    const int *const ell = sparse ? c->d_exps_ell.get() : c->d_exp_ell.get();
    const double *const res = sparse ? c->d_exps_r.get() : c->d_exp_r.get();
    const size_t nk = static_cast<size_t>(K), k4 = (nk + pass - 1) / pass * pass;
    const size_t state_words = k4 * 2 * Zs, part_words = static_cast<size_t>(nseg) * 3 * cpm::kElvNB * Zs, zone_words = nk * 2 * Z;
    if ((rc = elv_reserve(c->d_elv_ws, 2 * state_words + part_words + zone_words, "the workspace")) != CPM_OK) return rc;
    double *const ws_st[2] = {c->d_elv_ws, c->d_elv_ws + state_words};
    double *const part = c->d_elv_ws + 2 * state_words;
    if (!zone) zone = part + part_words;
    const size_t zt = static_cast<size_t>(Z) * T, cot_stride = 2 * zt;
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0, steps = pre + T;
    for (int s = steps - 1; s >= 0; --s) {
        const int t = s < pre ? s : s - pre, j = s - pre;
        const size_t row = static_cast<size_t>(t) * Z;
        const double *p_t = sparse ? nullptr : c->d_p + row * Z;
        const bool have = s != steps - 1;  // (false: mu = nu = 0 by construction, no product is formed)
        for (int f0 = 0; f0 < K; f0 += pass) {
            const int nf = std::min(K - f0, pass);
            const int NB = nf > 2 ? 4 : nf > 1 ? 2 : 1;
            const size_t w0 = static_cast<size_t>(f0) * 2 * Zs;
            const double *st = have ? ws_st[(s + 1) & 1] + w0 : nullptr;
            if (st && sparse) launch_exps_elv_u(c, NB, row, st, Zs, nseg, seg_len, nf, part);
            else if (st) launch_elv_u(c, NB, p_t, st, Zs, nseg, seg_len, nf, part);
            const double *gp = j >= 0 ? coeff + f0 * cot_stride + static_cast<size_t>(j) * Z : nullptr;
            const double *gd = j >= 0 ? gp + zt : nullptr;
            cpm::launch(cpm::k_elv_finish, dim3(nblk(Z, cpm::kFinishBlock), static_cast<unsigned>(NB)), dim3(cpm::kFinishBlock), 0, c->stream,
                        static_cast<const double *>(part), nseg, Zs, static_cast<const double *>(c->d_last + row), ell + row, res + row,
                        static_cast<const double *>(c->d_pdrive) + row, st, NB, gp, gd, cot_stride, Z, nf,
                        ws_st[s & 1] + w0, s == 0 ? zone + static_cast<size_t>(f0) * 2 * Z : static_cast<double *>(nullptr));
        }
        HIP_TRY(hipGetLastError());
    }
    cpm::launch(cpm::k_elv_total, dim3(2, static_cast<unsigned>(K)), dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(zone), d_start, Z, out);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

int32_t elv_enter(cpm_ctx *c, uint32_t flags, int32_t K)
{
    int32_t rc = exp_flags_check(flags);
    if (rc != CPM_OK) return rc;
    if (K < 1 || K > CPM_MAX_BATCH) return fail(CPM_ERR_ARG, "expected_linear_var: K = %d outside 1..%d", K, CPM_MAX_BATCH);
    CTX_TRY(c);
    if (!c->have_pdrive) return fail(CPM_ERR_STATE, "expected_linear_var: p_drive not set");
    return CPM_OK;
}

int32_t expected_linear_var_dev(cpm_ctx *c, const void *d_start, uint32_t flags, int32_t K, const void *d_coeff, void *d_out, void *d_zone, bool sparse)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_coeff) return fail(CPM_ERR_ARG, "expected_linear_var_dev: null d_coeff");
    if (!d_out) return fail(CPM_ERR_ARG, "expected_linear_var_dev: null d_out");
    if ((rc = elv_enter(c, flags, K)) != CPM_OK) return rc;
    if (sparse && (rc = exps_rows_ready(c, "expected_linear_var")) != CPM_OK) return rc;
    return expected_linear_var_enqueue(c, static_cast<const double *>(d_start), flags, K, static_cast<const double *>(d_coeff), static_cast<double *>(d_out),
                                       static_cast<double *>(d_zone), sparse);
}

// the blocking call: the checks of the host arrays, the copies in, the pass and the copies out (dense and sparse entries share it)
int32_t expected_linear_var_blocking(cpm_ctx *c, const double *start, uint32_t flags, int32_t K, const double *a_parking, const double *b_driving,
                                     double *mean, double *var, double *zone_mean, double *zone_var, bool sparse)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!a_parking || !b_driving) return fail(CPM_ERR_ARG, "expected_linear_var: null coefficients");
    if (!mean || !var) return fail(CPM_ERR_ARG, "expected_linear_var: null mean or var");
    if ((rc = elv_enter(c, flags, K)) != CPM_OK) return rc;
    if (sparse && (rc = exps_rows_ready(c, "expected_linear_var")) != CPM_OK) return rc;  // (state is refused before a coefficient is read or copied)
    const size_t Z = static_cast<size_t>(c->Z), zt = Z * static_cast<size_t>(c->T), nk = static_cast<size_t>(K);
    if (start)
        for (size_t z = 0; z < Z; ++z)
            if (!std::isfinite(start[z]) || start[z] < 0.0)
                return fail(CPM_ERR_ARG, "expected_linear_var: start of zone %lld is NaN, infinite or negative", (long long)z + 1);
    for (size_t i = 0; i < nk * zt; ++i)
        if (!std::isfinite(a_parking[i]) || !std::isfinite(b_driving[i]))
            return fail(CPM_ERR_ARG, "expected_linear_var: the coefficient of functional %lld, zone %lld, hour %lld is not finite", (long long)(i / zt) + 1,
                        (long long)(i % Z) + 1, (long long)(i % zt / Z) + 1);
    if ((rc = elv_reserve(c->d_elv_io, nk * (2 * zt + 2 + 2 * Z) + Z, "the blocking call's arrays")) != CPM_OK) return rc;
    double *const d_coeff = c->d_elv_io, *const d_out = d_coeff + nk * 2 * zt, *const d_zone = d_out + nk * 2, *const d_w = d_zone + nk * 2 * Z;
    for (size_t k = 0; k < nk; ++k) {
        HIP_TRY(hipMemcpyAsync(d_coeff + k * 2 * zt, a_parking + k * zt, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_coeff + k * 2 * zt + zt, b_driving + k * zt, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
    }
    if (start) HIP_TRY(hipMemcpyAsync(d_w, start, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    if ((rc = expected_linear_var_enqueue(c, start ? d_w : nullptr, flags, K, d_coeff, d_out, d_zone, sparse)) != CPM_OK) return rc;
    std::vector<double> h_out(nk * 2);
    HIP_TRY(hipMemcpyAsync(h_out.data(), d_out, sizeof(double) * nk * 2, hipMemcpyDeviceToHost, c->stream));
    for (size_t k = 0; k < nk; ++k) {
        if (zone_mean) HIP_TRY(hipMemcpyAsync(zone_mean + k * Z, d_zone + k * 2 * Z, sizeof(double) * Z, hipMemcpyDeviceToHost, c->stream));
        if (zone_var) HIP_TRY(hipMemcpyAsync(zone_var + k * Z, d_zone + k * 2 * Z + Z, sizeof(double) * Z, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < nk; ++k) mean[k] = h_out[2 * k], var[k] = h_out[2 * k + 1];
    return CPM_OK;
}

}  // namespace

int32_t cpm_expected_linear_var_dev(cpm_ctx *c, const void *d_start, uint32_t flags, int32_t K, const void *d_coeff, void *d_out, void *d_zone)
{
    return expected_linear_var_dev(c, d_start, flags, K, d_coeff, d_out, d_zone, false);
}

int32_t cpm_expected_linear_var(cpm_ctx *c, const double *start, uint32_t flags, int32_t K, const double *a_parking, const double *b_driving, double *mean,
                                double *var, double *zone_mean, double *zone_var)
{
    return expected_linear_var_blocking(c, start, flags, K, a_parking, b_driving, mean, var, zone_mean, zone_var, false);
}

// ------------------------------------------------------------------ the variance of travel functionals (include/cpm_expected_travel_var.h)

namespace {

int32_t etv_reserve(DevBuf<double> &b, size_t words, const char *what)
{
    if (b.reserve(words) == hipSuccess) return CPM_OK;
    (void)hipGetLastError();
    return fail(CPM_ERR_NOMEM, "expected_travel_var: cannot allocate %s: %zu bytes asked for", what, words * sizeof(double));
}

// The trip variance weights of the installed p_destin tables and datamatrix in d_exp_vsec: once per build of the trip weights
// (ensure_exp_trip reports a missing table, datamatrix or distance matrix and rebuilds under every condition these share).
// sparse: the weights of the compact rows in d_exps_vsec, once per build of the sparse trip weights (ensure_exps_trip): d_p is neither
// read nor built, and neither d_exp_vsec nor exp_tvar_builds moves.
int32_t ensure_exp_trip_var(cpm_ctx *c, bool sparse = false)
{
    if (sparse) {
        int32_t rc = ensure_exps_trip(c);
        if (rc != CPM_OK) return rc;
        if (c->exps_tvar_trip_build == c->exps_trip_builds) return CPM_OK;
        const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
        const size_t zt = static_cast<size_t>(Z) * T, plane = zt * Z;
        const int nseg = cpm::trip_segments(Z, T), seg_len = cpm::trip_segment_len(Z, nseg);
        if ((rc = etv_reserve(c->d_exps_vsec, zt, "the trip variance weights")) != CPM_OK) return rc;
        HIP_TRY(c->d_exp_wpart.reserve(2 * zt * nseg));  // (scratch of every build of trip weights: nothing reads it afterwards)
        const double *mean = c->d_dm.get(), *sdev = mean + plane;
        cpm::launch(cpm::k_exps_trip_var, dim3(static_cast<unsigned>(Z), static_cast<unsigned>(T)), dim3(cpm::kExpsGradBlock), 0, c->stream,
                    static_cast<const double *>(c->d_sp.get()), static_cast<const uint32_t *>(c->d_sj.get()), static_cast<const uint32_t *>(c->d_scnt.get()),
                    cpm::kDsCap, mean, sdev, Z, T, seg_len, nseg, c->d_exp_wpart.get());
        HIP_TRY(hipGetLastError());
        cpm::launch(cpm::k_exp_trip_var_finish, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T)), dim3(cpm::kExpBlock), 0, c->stream,
                    static_cast<const double *>(c->d_exp_wpart.get()), nseg, mean, sdev, static_cast<const double *>(c->d_last),
                    static_cast<const int *>(c->d_exps_ell.get()), static_cast<const double *>(c->d_exps_r.get()), Z, T, c->d_exps_vsec.get());
        HIP_TRY(hipGetLastError());
        c->exps_tvar_trip_build = c->exps_trip_builds;
        ++c->exps_tvar_builds;
        return CPM_OK;
    }
    int32_t rc = ensure_exp_trip(c);
    if (rc != CPM_OK) return rc;
    if ((rc = ensure_dense_p(c)) != CPM_OK) return rc;  // (the callers read d_p)
    if (c->exp_tvar_trip_build == c->exp_trip_builds) return CPM_OK;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const size_t zt = static_cast<size_t>(Z) * T, plane = zt * Z;
    const int nseg = cpm::trip_segments(Z, T), seg_len = cpm::trip_segment_len(Z, nseg);
    if ((rc = etv_reserve(c->d_exp_vsec, zt, "the trip variance weights")) != CPM_OK) return rc;
    HIP_TRY(c->d_exp_wpart.reserve(2 * zt * nseg));  // (scratch of every build of trip weights: nothing reads it afterwards)
    const double *mean = c->d_dm.get(), *sdev = mean + plane;
    const dim3 grid(nblk(Z, cpm::kTripStrip), static_cast<unsigned>(T), static_cast<unsigned>(nseg));
    if (Z & 1) cpm::launch(cpm::k_exp_trip_var<true>, grid, dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(c->d_p.get()), mean, sdev, Z, T,
                           seg_len, c->d_exp_wpart.get());
    else cpm::launch(cpm::k_exp_trip_var<false>, grid, dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(c->d_p.get()), mean, sdev, Z, T,
                     seg_len, c->d_exp_wpart.get());
    HIP_TRY(hipGetLastError());
    cpm::launch(cpm::k_exp_trip_var_finish, dim3(nblk(Z, cpm::kExpBlock), static_cast<unsigned>(T)), dim3(cpm::kExpBlock), 0, c->stream,
                static_cast<const double *>(c->d_exp_wpart.get()), nseg, mean, sdev, static_cast<const double *>(c->d_last),
                static_cast<const int *>(c->d_exp_ell.get()), static_cast<const double *>(c->d_exp_r.get()), Z, T, c->d_exp_vsec.get());
    HIP_TRY(hipGetLastError());
    c->exp_tvar_trip_build = c->exp_trip_builds;
    ++c->exp_tvar_builds;
    return CPM_OK;
}

// one backward product of a pass: the smallest instantiation that holds it
void launch_etv_u(cpm_ctx *c, int NB, const double *p_t, const double *m_t, const double *st, const double *cs, const double *cd, size_t cot_stride, int Zs,
                  int nseg, int seg_len, int nf, double *part)
{
    const int Z = static_cast<int>(c->Z);
    const dim3 grid(nblk(Z, cpm::kGradStrip), static_cast<unsigned>(nseg)), block(cpm::kExpBlock);
    const auto k = NB == 2 ? ((Z & 1) ? cpm::k_etv_u<2, true> : cpm::k_etv_u<2, false>) : ((Z & 1) ? cpm::k_etv_u<1, true> : cpm::k_etv_u<1, false>);
    cpm::launch(k, grid, block, 0, c->stream, p_t, m_t, static_cast<const double *>(c->d_dist.get()), st, cs, cd, cot_stride, Z, Zs, seg_len, nf, part);
}

// ... from the compact rows of the hour whose first row is `row` (k_exps_etv_u<NB>; ensure_exps has run)
void launch_exps_etv_u(cpm_ctx *c, int NB, size_t row, const double *m_t, const double *st, const double *cs, const double *cd, size_t cot_stride, int Zs,
                       int nseg, int seg_len, int nf, double *part)
{
    const int Z = static_cast<int>(c->Z);
    const auto k = NB == 2 ? cpm::k_exps_etv_u<2> : cpm::k_exps_etv_u<1>;
    cpm::launch(k, dim3(static_cast<unsigned>(Z)), dim3(cpm::kExpsGradBlock), 0, c->stream, static_cast<const double *>(c->d_sp + row * cpm::kDsCap),
                static_cast<const uint32_t *>(c->d_sj + row * cpm::kDsCap), static_cast<const uint32_t *>(c->d_scnt + row), cpm::kDsCap, m_t,
                static_cast<const double *>(c->d_dist.get()), st, cs, cd, cot_stride, Z, Zs, seg_len, nseg, nf, part);
}

// The backward pass for K functionals, operator-major with the passes of at most kEtvNB functionals inside an operator, then the
// weighted totals: enqueued on the context's stream.  coeff: [K][4][T][Z] (A, B, S, D); out: [K][2]; zone: [K][2][Z] or nullptr.
// d_etv_ws, in vectors of Zs words: the state ping and pong, [K2][2] each (K2 = K rounded up to whole passes; a pass's state is
// [Zs][2][NB] at its first functional's place), the segments' sums [nseg][3][kEtvNB], and [K][2][Z] words where zone is nullptr.
// The state behind the last operator is zeroed and its product is formed like every other: zeta = e there.
// sparse: the products read the compact rows (k_exps_etv_u), the per-table arrays of ensure_exps and the weights of d_exps_vsec; d_p is
// neither read nor built.
int32_t expected_travel_var_enqueue(cpm_ctx *c, const double *d_start, uint32_t flags, int K, const double *coeff, double *out, double *zone,
                                    bool sparse = false)
{
    int32_t rc = ensure_exp_trip_var(c, sparse);  // (the tables, the datamatrix and the distances; dense: expands sparse tables to the dense array)
    if (rc != CPM_OK) return rc;
    const int Z = static_cast<int>(c->Z), T = static_cast<int>(c->T);
    const int Zs = (Z + 1) & ~1;
    const int nseg = cpm::grad_segments(Z), seg_len = cpm::grad_segment_len(Z, nseg);
    const int *const ell = sparse ? c->d_exps_ell.get() : c->d_exp_ell.get();
    const double *const res = sparse ? c->d_exps_r.get() : c->d_exp_r.get();
    const double *const vsec = sparse ? c->d_exps_vsec.get() : c->d_exp_vsec.get();
    const size_t nk = static_cast<size_t>(K), k2 = (nk + cpm::kEtvNB - 1) / cpm::kEtvNB * cpm::kEtvNB;
    const size_t state_words = k2 * 2 * Zs, part_words = static_cast<size_t>(nseg) * 3 * cpm::kEtvNB * Zs, zone_words = nk * 2 * Z;
    if ((rc = etv_reserve(c->d_etv_ws, 2 * state_words + part_words + zone_words, "the workspace")) != CPM_OK) return rc;
    double *const ws_st[2] = {c->d_etv_ws, c->d_etv_ws + state_words};
    double *const part = c->d_etv_ws + 2 * state_words;
    if (!zone) zone = part + part_words;
    const size_t zt = static_cast<size_t>(Z) * T, cot_stride = 4 * zt;
    const int pre = (flags & CPM_EXPECT_IVP) ? T - 1 : 0, steps = pre + T;
    HIP_TRY(hipMemsetAsync(ws_st[steps & 1], 0, sizeof(double) * state_words, c->stream));  // mu = nu = 0 behind the last operator
    for (int s = steps - 1; s >= 0; --s) {
        const int t = s < pre ? s : s - pre, j = s - pre;
        const size_t row = static_cast<size_t>(t) * Z;
        const double *p_t = sparse ? nullptr : c->d_p + row * Z, *m_t = c->d_dm + row * Z;
        for (int f0 = 0; f0 < K; f0 += cpm::kEtvNB) {
            const int nf = std::min(K - f0, cpm::kEtvNB);
            const int NB = nf > 1 ? 2 : 1;
            const size_t w0 = static_cast<size_t>(f0) * 2 * Zs;
            const double *st = ws_st[(s + 1) & 1] + w0;
            const double *gp = j >= 0 ? coeff + f0 * cot_stride + static_cast<size_t>(j) * Z : nullptr;
            const double *gd = j >= 0 ? gp + zt : nullptr, *cs = j >= 0 ? gp + 2 * zt : nullptr, *cd = j >= 0 ? gp + 3 * zt : nullptr;
            if (sparse) launch_exps_etv_u(c, NB, row, m_t, st, cs, cd, cot_stride, Zs, nseg, seg_len, nf, part);
            else launch_etv_u(c, NB, p_t, m_t, st, cs, cd, cot_stride, Zs, nseg, seg_len, nf, part);
            cpm::launch(cpm::k_etv_finish, dim3(nblk(Z, cpm::kFinishBlock), static_cast<unsigned>(NB)), dim3(cpm::kFinishBlock), 0, c->stream,
                        static_cast<const double *>(part), nseg, Zs, static_cast<const double *>(c->d_last + row), ell + row, res + row,
                        static_cast<const double *>(c->d_pdrive) + row, m_t, static_cast<const double *>(c->d_dist.get()), vsec + row, st, NB, gp, gd, cs, cd,
                        cot_stride, Z, nf, ws_st[s & 1] + w0, s == 0 ? zone + static_cast<size_t>(f0) * 2 * Z : static_cast<double *>(nullptr));
        }
        HIP_TRY(hipGetLastError());
    }
    cpm::launch(cpm::k_elv_total, dim3(2, static_cast<unsigned>(K)), dim3(cpm::kExpBlock), 0, c->stream, static_cast<const double *>(zone), d_start, Z, out);
    HIP_TRY(hipGetLastError());
    return CPM_OK;
}

int32_t etv_enter(cpm_ctx *c, uint32_t flags, int32_t K)
{
    int32_t rc = exp_flags_check(flags);
    if (rc != CPM_OK) return rc;
    if (K < 1 || K > CPM_MAX_BATCH) return fail(CPM_ERR_ARG, "expected_travel_var: K = %d outside 1..%d", K, CPM_MAX_BATCH);
    CTX_TRY(c);
    if (!c->have_pdrive) return fail(CPM_ERR_STATE, "expected_travel_var: p_drive not set");
    return CPM_OK;
}

// v_sec to a device (to_host false) or a host array; sparse: the weights of the compact rows
int32_t expected_trip_var_copy(cpm_ctx *c, void *v, bool to_host, bool sparse)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!v) return to_host ? fail(CPM_ERR_ARG, "expected_trip_var: null v_sec") : fail(CPM_ERR_ARG, "expected_trip_var_dev: null d_v");
    CTX_TRY(c);
    if (sparse && (rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;
    if ((rc = ensure_exp_trip_var(c, sparse)) != CPM_OK) return rc;
    const double *const src = sparse ? c->d_exps_vsec.get() : c->d_exp_vsec.get();
    HIP_TRY(hipMemcpyAsync(v, src, sizeof(double) * c->Z * c->T, to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    if (to_host) HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t expected_travel_var_dev(cpm_ctx *c, const void *d_start, uint32_t flags, int32_t K, const void *d_coeff, void *d_out, void *d_zone, bool sparse)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_coeff) return fail(CPM_ERR_ARG, "expected_travel_var_dev: null d_coeff");
    if (!d_out) return fail(CPM_ERR_ARG, "expected_travel_var_dev: null d_out");
    if ((rc = etv_enter(c, flags, K)) != CPM_OK) return rc;
    if (sparse && (rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;
    return expected_travel_var_enqueue(c, static_cast<const double *>(d_start), flags, K, static_cast<const double *>(d_coeff), static_cast<double *>(d_out),
                                       static_cast<double *>(d_zone), sparse);
}

// the blocking call: the checks of the host arrays, the copies in, the pass and the copies out (dense and sparse entries share it)
int32_t expected_travel_var_blocking(cpm_ctx *c, const double *start, uint32_t flags, int32_t K, const double *a_parking, const double *b_driving,
                                     const double *s_seconds, const double *d_km, double *mean, double *var, double *zone_mean, double *zone_var,
                                     bool sparse)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!a_parking || !b_driving) return fail(CPM_ERR_ARG, "expected_travel_var: null coefficients");
    if (!mean || !var) return fail(CPM_ERR_ARG, "expected_travel_var: null mean or var");
    if ((rc = etv_enter(c, flags, K)) != CPM_OK) return rc;
    if (sparse && (rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;  // (state is refused before a coefficient is read or copied)
    const size_t Z = static_cast<size_t>(c->Z), zt = Z * static_cast<size_t>(c->T), nk = static_cast<size_t>(K);
    if (start)
        for (size_t z = 0; z < Z; ++z)
            if (!std::isfinite(start[z]) || start[z] < 0.0)
                return fail(CPM_ERR_ARG, "expected_travel_var: start of zone %lld is NaN, infinite or negative", (long long)z + 1);
    const double *const host[4] = {a_parking, b_driving, s_seconds, d_km};
    for (size_t i = 0; i < nk * zt; ++i)
        for (int a = 0; a < 4; ++a)
            if (host[a] && !std::isfinite(host[a][i]))
                return fail(CPM_ERR_ARG, "expected_travel_var: the coefficient of functional %lld, zone %lld, hour %lld is not finite", (long long)(i / zt) + 1,
                            (long long)(i % Z) + 1, (long long)(i % zt / Z) + 1);
    if ((rc = etv_reserve(c->d_etv_io, nk * (4 * zt + 2 + 2 * Z) + Z, "the blocking call's arrays")) != CPM_OK) return rc;
    double *const d_coeff = c->d_etv_io, *const d_out = d_coeff + nk * 4 * zt, *const d_zone = d_out + nk * 2, *const d_w = d_zone + nk * 2 * Z;
    for (size_t k = 0; k < nk; ++k)
        for (int a = 0; a < 4; ++a) {
            double *const dst = d_coeff + (k * 4 + a) * zt;
            if (host[a]) HIP_TRY(hipMemcpyAsync(dst, host[a] + k * zt, sizeof(double) * zt, hipMemcpyHostToDevice, c->stream));
            else HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * zt, c->stream));  // (a NULL trip array: zeros)
        }
    if (start) HIP_TRY(hipMemcpyAsync(d_w, start, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    if ((rc = expected_travel_var_enqueue(c, start ? d_w : nullptr, flags, K, d_coeff, d_out, d_zone, sparse)) != CPM_OK) return rc;
    std::vector<double> h_out(nk * 2);
    HIP_TRY(hipMemcpyAsync(h_out.data(), d_out, sizeof(double) * nk * 2, hipMemcpyDeviceToHost, c->stream));
    for (size_t k = 0; k < nk; ++k) {
        if (zone_mean) HIP_TRY(hipMemcpyAsync(zone_mean + k * Z, d_zone + k * 2 * Z, sizeof(double) * Z, hipMemcpyDeviceToHost, c->stream));
        if (zone_var) HIP_TRY(hipMemcpyAsync(zone_var + k * Z, d_zone + k * 2 * Z + Z, sizeof(double) * Z, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < nk; ++k) mean[k] = h_out[2 * k], var[k] = h_out[2 * k + 1];
    return CPM_OK;
}

}  // namespace

int32_t cpm_expected_trip_var_dev(cpm_ctx *c, void *d_v)
{
    return expected_trip_var_copy(c, d_v, false, false);
}

int32_t cpm_expected_trip_var(cpm_ctx *c, double *v_sec)
{
    return expected_trip_var_copy(c, v_sec, true, false);
}

int64_t cpm_expected_trip_var_builds(const cpm_ctx *c)
{
    const int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    return c->exp_tvar_builds;
}

int32_t cpm_expected_travel_var_dev(cpm_ctx *c, const void *d_start, uint32_t flags, int32_t K, const void *d_coeff, void *d_out, void *d_zone)
{
    return expected_travel_var_dev(c, d_start, flags, K, d_coeff, d_out, d_zone, false);
}

int32_t cpm_expected_travel_var(cpm_ctx *c, const double *start, uint32_t flags, int32_t K, const double *a_parking, const double *b_driving,
                                const double *s_seconds, const double *d_km, double *mean, double *var, double *zone_mean, double *zone_var)
{
    return expected_travel_var_blocking(c, start, flags, K, a_parking, b_driving, s_seconds, d_km, mean, var, zone_mean, zone_var, false);
}

// ------------------------------------------------------------------ the same variances from the compact rows (include/cpm_expected_sparse_var.h):
// the namesakes' bodies with sparse = true, and CPM_ERR_STATE without compact rows in front of anything that is read, copied or enqueued

int32_t cpm_expected_sparse_linear_var_dev(cpm_ctx *c, const void *d_start, uint32_t flags, int32_t K, const void *d_coeff, void *d_out, void *d_zone)
{
    return expected_linear_var_dev(c, d_start, flags, K, d_coeff, d_out, d_zone, true);
}

int32_t cpm_expected_sparse_linear_var(cpm_ctx *c, const double *start, uint32_t flags, int32_t K, const double *a_parking, const double *b_driving,
                                       double *mean, double *var, double *zone_mean, double *zone_var)
{
    return expected_linear_var_blocking(c, start, flags, K, a_parking, b_driving, mean, var, zone_mean, zone_var, true);
}

int32_t cpm_expected_sparse_trip_var_dev(cpm_ctx *c, void *d_v)
{
    return expected_trip_var_copy(c, d_v, false, true);
}

int32_t cpm_expected_sparse_trip_var(cpm_ctx *c, double *v_sec)
{
    return expected_trip_var_copy(c, v_sec, true, true);
}

int64_t cpm_expected_sparse_trip_var_builds(const cpm_ctx *c)
{
    const int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    return c->exps_tvar_builds;
}

int32_t cpm_expected_sparse_travel_var_dev(cpm_ctx *c, const void *d_start, uint32_t flags, int32_t K, const void *d_coeff, void *d_out, void *d_zone)
{
    return expected_travel_var_dev(c, d_start, flags, K, d_coeff, d_out, d_zone, true);
}

int32_t cpm_expected_sparse_travel_var(cpm_ctx *c, const double *start, uint32_t flags, int32_t K, const double *a_parking, const double *b_driving,
                                       const double *s_seconds, const double *d_km, double *mean, double *var, double *zone_mean, double *zone_var)
{
    return expected_travel_var_blocking(c, start, flags, K, a_parking, b_driving, s_seconds, d_km, mean, var, zone_mean, zone_var, true);
}

// ------------------------------------------------------------------ the same from sparse tables (include/cpm_expected_sparse.h)

int32_t cpm_expected_sparse_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, void *d_out, void *d_pi_next)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_out) return fail(CPM_ERR_ARG, "expected_sparse_dev: null d_out");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<double *>(d_out),
                            static_cast<double *>(d_pi_next), true);
}

int32_t cpm_expected_sparse_batch_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, void *d_out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_out) return fail(CPM_ERR_ARG, "expected_sparse_batch_dev: null d_out");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    return expected_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<double *>(d_out), nullptr, true);
}

int32_t cpm_expected_sparse(cpm_ctx *c, const double *pi0, uint32_t flags, double *parking, double *driving, double *pi_next)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!parking || !driving) return fail(CPM_ERR_ARG, "expected_sparse: null density outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, parking, driving, pi_next, true);
}

int32_t cpm_expected_sparse_batch(cpm_ctx *c, const double *pi0, uint32_t flags, double *parking, double *driving)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!parking || !driving) return fail(CPM_ERR_ARG, "expected_sparse_batch: null density outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    return expected_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, parking, driving, nullptr, true);
}

int32_t cpm_expected_sparse_aux(cpm_ctx *c, int32_t sparse, int32_t *ell, double *r, int32_t *start, int32_t *list)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!ell || !r || !start || !list) return fail(CPM_ERR_ARG, "expected_sparse_aux: null outputs");
    CTX_TRY(c);
    if ((rc = exp_tables_ready(c, "expected_sparse_aux")) != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps(c) : ensure_exp_aux(c)) != CPM_OK) return rc;
    const size_t rows = static_cast<size_t>(c->Z) * c->T;
    HIP_TRY(hipMemcpyAsync(ell, sparse ? c->d_exps_ell.get() : c->d_exp_ell.get(), sizeof(int) * rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(r, sparse ? c->d_exps_r.get() : c->d_exp_r.get(), sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(start, sparse ? c->d_exps_start.get() : c->d_exp_start.get(), sizeof(int) * (rows + c->T), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(list, sparse ? c->d_exps_list.get() : c->d_exp_list.get(), sizeof(int) * rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ the adjoint, the trip weights and the fit from the compact rows
// (include/cpm_expected_sparse_grad.h): the namesakes' entries with sparse = true, and CPM_ERR_STATE without compact rows in front of
// anything that is read, copied or enqueued
static int32_t exps_rows_ready(const cpm_ctx *c, const char *what)
{
    int32_t rc = exp_tables_ready(c, what);
    if (rc != CPM_OK) return rc;
    return c->sparse_tables ? CPM_OK : exps_no_rows();
}

int32_t cpm_expected_sparse_grad_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext, void *d_grad_p_drive,
                                     void *d_grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_sparse_grad_dev: null d_cotangent");
    if (!d_grad_p_drive) return fail(CPM_ERR_ARG, "expected_sparse_grad_dev: null d_grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;
    return expected_grad_enqueue(c, static_cast<const double *>(d_pi0), flags, static_cast<const double *>(d_cotangent), static_cast<const double *>(d_gnext),
                                 static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0), true);
}

int32_t cpm_expected_sparse_grad(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                                 double *grad_p_drive, double *grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_sparse_grad: null cotangents");
    if (!grad_p_drive) return fail(CPM_ERR_ARG, "expected_sparse_grad: null grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;
    return expected_grad_blocking(c, pi0, flags, g_parking, g_driving, g_next, grad_p_drive, grad_pi0, true);
}

int32_t cpm_expected_sparse_grad_batch_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext, void *d_grad_p_drive,
                                           void *d_grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_sparse_grad_batch_dev: null d_cotangent");
    if (!d_grad_p_drive) return fail(CPM_ERR_ARG, "expected_sparse_grad_batch_dev: null d_grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;
    return expected_grad_batch_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<const double *>(d_cotangent),
                                       static_cast<const double *>(d_gnext), static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0), nullptr,
                                       true);
}

int32_t cpm_expected_sparse_grad_batch(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                                       double *grad_p_drive, double *grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_sparse_grad_batch: null cotangents");
    if (!grad_p_drive) return fail(CPM_ERR_ARG, "expected_sparse_grad_batch: null grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;  // (state is refused before a cotangent is read or copied)
    return expected_grad_batch_blocking(c, "expected_sparse_grad_batch", pi0, flags, tb.B, tb.pd, tb.q_stride, g_parking, g_driving, g_next, grad_p_drive,
                                        grad_pi0, nullptr, true);
}

int32_t cpm_expected_sparse_trip_dev(cpm_ctx *c, void *d_w)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_w) return fail(CPM_ERR_ARG, "expected_sparse_trip_dev: null d_w");
    CTX_TRY(c);
    if ((rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;
    if ((rc = ensure_exps_trip(c)) != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_w, c->d_exps_w, sizeof(double) * 2 * c->Z * c->T, hipMemcpyDeviceToDevice, c->stream));
    return CPM_OK;
}

int32_t cpm_expected_sparse_trip(cpm_ctx *c, double *w_sec, double *w_km)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!w_sec || !w_km) return fail(CPM_ERR_ARG, "expected_sparse_trip: null outputs");
    CTX_TRY(c);
    if ((rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;
    if ((rc = ensure_exps_trip(c)) != CPM_OK) return rc;
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    HIP_TRY(hipMemcpyAsync(w_sec, c->d_exps_w, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(w_km, c->d_exps_w + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_expected_sparse_travel_dev(cpm_ctx *c, const void *d_expected, int32_t B, void *d_travel, void *d_totals)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_expected) return fail(CPM_ERR_ARG, "expected_sparse_travel_dev: null d_expected");
    if (B < 1) return fail(CPM_ERR_ARG, "expected_sparse_travel_dev: B = %d", B);
    if (!d_travel && !d_totals) return fail(CPM_ERR_ARG, "expected_sparse_travel_dev: d_travel and d_totals are both null");
    CTX_TRY(c);
    if ((rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;
    return expected_travel_enqueue(c, static_cast<const double *>(d_expected), B, static_cast<double *>(d_travel), static_cast<double *>(d_totals), true);
}

int32_t cpm_expected_sparse_travel(cpm_ctx *c, const double *pi0, uint32_t flags, double *seconds, double *km, double *totals)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!seconds || !km) return fail(CPM_ERR_ARG, "expected_sparse_travel: null outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;
    return expected_travel_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, seconds, km, totals, true);
}

int32_t cpm_expected_sparse_travel_batch(cpm_ctx *c, const double *pi0, uint32_t flags, double *seconds, double *km, double *totals)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!seconds || !km) return fail(CPM_ERR_ARG, "expected_sparse_travel_batch: null outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected travel")) != CPM_OK) return rc;
    return expected_travel_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, seconds, km, totals, true);
}

// ------------------------------------------------------------------ expected travel (include/cpm_expected_travel.h)

int32_t cpm_expected_trip_dev(cpm_ctx *c, void *d_w)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_w) return fail(CPM_ERR_ARG, "expected_trip_dev: null d_w");
    CTX_TRY(c);
    if ((rc = ensure_exp_trip(c)) != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_w, c->d_exp_w, sizeof(double) * 2 * c->Z * c->T, hipMemcpyDeviceToDevice, c->stream));
    return CPM_OK;
}

int32_t cpm_expected_trip(cpm_ctx *c, double *w_sec, double *w_km)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!w_sec || !w_km) return fail(CPM_ERR_ARG, "expected_trip: null outputs");
    CTX_TRY(c);
    if ((rc = ensure_exp_trip(c)) != CPM_OK) return rc;
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    HIP_TRY(hipMemcpyAsync(w_sec, c->d_exp_w, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(w_km, c->d_exp_w + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_expected_travel_dev(cpm_ctx *c, const void *d_expected, int32_t B, void *d_travel, void *d_totals)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_expected) return fail(CPM_ERR_ARG, "expected_travel_dev: null d_expected");
    if (B < 1) return fail(CPM_ERR_ARG, "expected_travel_dev: B = %d", B);
    if (!d_travel && !d_totals) return fail(CPM_ERR_ARG, "expected_travel_dev: d_travel and d_totals are both null");
    CTX_TRY(c);
    return expected_travel_enqueue(c, static_cast<const double *>(d_expected), B, static_cast<double *>(d_travel), static_cast<double *>(d_totals));
}

int32_t cpm_expected_travel(cpm_ctx *c, const double *pi0, uint32_t flags, double *seconds, double *km, double *totals)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!seconds || !km) return fail(CPM_ERR_ARG, "expected_travel: null outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_travel_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, seconds, km, totals);
}

int32_t cpm_expected_travel_batch(cpm_ctx *c, const double *pi0, uint32_t flags, double *seconds, double *km, double *totals)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!seconds || !km) return fail(CPM_ERR_ARG, "expected_travel_batch: null outputs");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    return expected_travel_blocking(c, pi0, flags, tb.B, tb.pd, tb.q_stride, seconds, km, totals);
}

int64_t cpm_expected_trip_builds(const cpm_ctx *c)
{
    const int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    return c->exp_trip_builds;
}

// ------------------------------------------------------------------ adjoint of the expected densities (include/cpm_expected_grad.h)

int32_t cpm_expected_grad_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext, void *d_grad_p_drive,
                              void *d_grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_grad_dev: null d_cotangent");
    if (!d_grad_p_drive) return fail(CPM_ERR_ARG, "expected_grad_dev: null d_grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_grad_enqueue(c, static_cast<const double *>(d_pi0), flags, static_cast<const double *>(d_cotangent), static_cast<const double *>(d_gnext),
                                 static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0));
}

int32_t cpm_expected_grad(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                          double *grad_p_drive, double *grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_grad: null cotangents");
    if (!grad_p_drive) return fail(CPM_ERR_ARG, "expected_grad: null grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_grad_blocking(c, pi0, flags, g_parking, g_driving, g_next, grad_p_drive, grad_pi0);
}

// ------------------------------------------------------------------ adjoint along a tangent of p_destin (include/cpm_expected_grad_dest.h)

int32_t cpm_set_p_dest_tangent(cpm_ctx *c, const double *dp)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!dp) return fail(CPM_ERR_ARG, "set_p_dest_tangent: null dp");
    CTX_TRY(c);
    if ((rc = exp_tables_ready(c, "set_p_dest_tangent")) != CPM_OK) return rc;
    const size_t Z = static_cast<size_t>(c->Z), cells = Z * Z * static_cast<size_t>(c->T);
    for (size_t i = 0; i < cells; ++i)
        if (!std::isfinite(dp[i]))
            return fail(CPM_ERR_ARG, "set_p_dest_tangent: the entry of origin %lld, destination %lld, hour %lld is not finite", (long long)(i % Z) + 1,
                        (long long)(i / Z % Z) + 1, (long long)(i / (Z * Z)) + 1);
    c->tan_valid = false;
    HIP_TRY(c->d_tan.reserve(cells));
    HIP_TRY(hipMemcpyAsync(c->d_tan, dp, sizeof(double) * cells, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tan_valid = true;
    ++c->tan_gen;
    return CPM_OK;
}

int32_t cpm_build_p_dest_tangent(cpm_ctx *c, double *out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    CTX_TRY(c);
    if ((rc = build_dest_tangent(c)) != CPM_OK) return rc;
    if (out) {
        HIP_TRY(hipMemcpyAsync(out, c->d_tan, sizeof(double) * c->Z * c->Z * c->T, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CPM_OK;
}

int32_t cpm_get_p_dest_tangent(cpm_ctx *c, double *out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!out) return fail(CPM_ERR_ARG, "get_p_dest_tangent: null out");
    CTX_TRY(c);
    if ((rc = tangent_ready(c, "get_p_dest_tangent")) != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_tan, sizeof(double) * c->Z * c->Z * c->T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_expected_grad_dest_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext, void *d_grad_p_drive,
                                   void *d_grad_pi0, void *d_grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_grad_dest_dev: null d_cotangent");
    if (!d_grad_p_drive || !d_grad_dest) return fail(CPM_ERR_ARG, "expected_grad_dest_dev: null d_grad_p_drive or d_grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    return expected_grad_dest_enqueue(c, static_cast<const double *>(d_pi0), flags, static_cast<const double *>(d_cotangent),
                                      static_cast<const double *>(d_gnext), static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0),
                                      static_cast<double *>(d_grad_dest));
}

int32_t cpm_expected_grad_dest(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                               double *grad_p_drive, double *grad_pi0, double *grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_grad_dest: null cotangents");
    if (!grad_p_drive || !grad_dest) return fail(CPM_ERR_ARG, "expected_grad_dest: null grad_p_drive or grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    if ((rc = exp_tables_ready(c, "expected")) != CPM_OK) return rc;  // (state is refused before a cotangent is read or copied)
    if ((rc = tangent_ready(c, "expected_grad_dest")) != CPM_OK) return rc;
    return expected_grad_dest_blocking(c, pi0, flags, g_parking, g_driving, g_next, grad_p_drive, grad_pi0, grad_dest);
}

// ------------------------------------------------------------------ the adjoint for the fleets of a batch (include/cpm_expected_grad_batch.h)
int32_t cpm_expected_grad_batch_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext, void *d_grad_p_drive,
                                    void *d_grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_grad_batch_dev: null d_cotangent");
    if (!d_grad_p_drive) return fail(CPM_ERR_ARG, "expected_grad_batch_dev: null d_grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    return expected_grad_batch_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<const double *>(d_cotangent),
                                       static_cast<const double *>(d_gnext), static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0), nullptr);
}

int32_t cpm_expected_grad_batch(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                                double *grad_p_drive, double *grad_pi0)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_grad_batch: null cotangents");
    if (!grad_p_drive) return fail(CPM_ERR_ARG, "expected_grad_batch: null grad_p_drive");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    if ((rc = exp_tables_ready(c, "expected")) != CPM_OK) return rc;  // (state is refused before a cotangent is read or copied)
    return expected_grad_batch_blocking(c, "expected_grad_batch", pi0, flags, tb.B, tb.pd, tb.q_stride, g_parking, g_driving, g_next, grad_p_drive, grad_pi0,
                                        nullptr);
}

int32_t cpm_expected_grad_dest_batch_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext, void *d_grad_p_drive,
                                         void *d_grad_pi0, void *d_grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_grad_dest_batch_dev: null d_cotangent");
    if (!d_grad_p_drive || !d_grad_dest) return fail(CPM_ERR_ARG, "expected_grad_dest_batch_dev: null d_grad_p_drive or d_grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    return expected_grad_batch_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<const double *>(d_cotangent),
                                       static_cast<const double *>(d_gnext), static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0),
                                       static_cast<double *>(d_grad_dest));
}

int32_t cpm_expected_grad_dest_batch(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                                     double *grad_p_drive, double *grad_pi0, double *grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_grad_dest_batch: null cotangents");
    if (!grad_p_drive || !grad_dest) return fail(CPM_ERR_ARG, "expected_grad_dest_batch: null grad_p_drive or grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    if ((rc = exp_tables_ready(c, "expected")) != CPM_OK) return rc;  // (state is refused before a cotangent is read or copied)
    if ((rc = tangent_ready(c, "expected_grad_dest_batch")) != CPM_OK) return rc;
    return expected_grad_batch_blocking(c, "expected_grad_dest_batch", pi0, flags, tb.B, tb.pd, tb.q_stride, g_parking, g_driving, g_next, grad_p_drive, grad_pi0,
                                        grad_dest);
}

int32_t cpm_expected_trip_tangent_dev(cpm_ctx *c, void *d_dw)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_dw) return fail(CPM_ERR_ARG, "expected_trip_tangent_dev: null d_dw");
    CTX_TRY(c);
    return trip_tangent_enqueue(c, static_cast<double *>(d_dw));
}

int32_t cpm_expected_trip_tangent(cpm_ctx *c, double *dw_sec, double *dw_km)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!dw_sec || !dw_km) return fail(CPM_ERR_ARG, "expected_trip_tangent: null outputs");
    CTX_TRY(c);
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    HIP_TRY(c->d_tan_w.reserve(2 * zt));
    if ((rc = trip_tangent_enqueue(c, c->d_tan_w)) != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dw_sec, c->d_tan_w, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dw_km, c->d_tan_w + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ value and gradient of the objectives (include/cpm_expected_fit.h)

int32_t cpm_set_measured_activity(cpm_ctx *c, const double *activity)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    CTX_TRY(c);
    if (!activity) {  // (host state only: what is in flight on the stream was enqueued with the data it had)
        c->have_act_meas = false;
        return CPM_OK;
    }
    for (int64_t t = 0; t < c->T; ++t)
        if (!std::isfinite(activity[t])) return fail(CPM_ERR_ARG, "set_measured_activity: hour %lld is not finite", (long long)t + 1);
    HIP_TRY(c->d_act_meas.reserve(static_cast<size_t>(c->T)));
    HIP_TRY(hipMemcpyAsync(c->d_act_meas, activity, sizeof(double) * c->T, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_act_meas = true;
    return CPM_OK;
}

int32_t cpm_expected_fit_dev(cpm_ctx *c, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const void *d_pi0, uint32_t flags,
                             const double *weights, void *d_record, void *d_expected, void *d_cotangent, void *d_grad_p_drive, void *d_grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if ((rc = fit_check(c, "expected_fit_dev", B, p_min, p_max, e_drive, flags, weights, d_record)) != CPM_OK) return rc;
    if (d_grad_dest && !(flags & CPM_FIT_DEST)) return fail(CPM_ERR_ARG, "expected_fit_dev: d_grad_dest without CPM_FIT_DEST");
    return expected_fit_enqueue(c, B, p_min, p_max, e_drive, static_cast<const double *>(d_pi0), flags, weights, static_cast<double *>(d_record),
                                static_cast<double *>(d_expected), static_cast<double *>(d_cotangent), static_cast<double *>(d_grad_p_drive),
                                static_cast<double *>(d_grad_dest));
}

// the blocking call behind its checks: pi_0 up, the call into the workspace, the outputs the caller wants down
static int32_t expected_fit_blocking(cpm_ctx *c, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const double *pi0, uint32_t flags,
                              const double *weights, double *record, double *expected, double *cotangent, double *grad_p_drive, double *grad_dest, bool sparse)
{
    int32_t rc = check_pi0(c, pi0);
    if (rc != CPM_OK) return rc;
    const size_t Z = static_cast<size_t>(c->Z), zt = Z * static_cast<size_t>(c->T), nb = static_cast<size_t>(B);
    const size_t rec_words = nb * static_cast<size_t>(cpm::kFitWords + c->T);
    HIP_TRY(c->d_fit_rec.reserve(rec_words + Z));
    double *d_pi0 = c->d_fit_rec + (c->d_fit_rec.cap - Z);  // (pi_0 ends the allocation)
    if (pi0) HIP_TRY(hipMemcpyAsync(d_pi0, pi0, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    rc = expected_fit_enqueue(c, B, p_min, p_max, e_drive, pi0 ? d_pi0 : nullptr, flags, weights, c->d_fit_rec, nullptr, nullptr, nullptr, nullptr, sparse);
    if (rc != CPM_OK) return rc;
    const FitLayout l = fit_layout(c, B);
    const double *ws = c->d_fit_ws;
    HIP_TRY(hipMemcpyAsync(record, c->d_fit_rec, sizeof(double) * rec_words, hipMemcpyDeviceToHost, c->stream));
    if (expected) HIP_TRY(hipMemcpyAsync(expected, ws + l.expected, sizeof(double) * nb * 2 * zt, hipMemcpyDeviceToHost, c->stream));
    if (cotangent) HIP_TRY(hipMemcpyAsync(cotangent, ws + l.cot, sizeof(double) * nb * 2 * zt, hipMemcpyDeviceToHost, c->stream));
    if (grad_p_drive) HIP_TRY(hipMemcpyAsync(grad_p_drive, ws + l.grad_pd, sizeof(double) * nb * zt, hipMemcpyDeviceToHost, c->stream));
    if (grad_dest && (flags & CPM_FIT_DEST)) HIP_TRY(hipMemcpyAsync(grad_dest, ws + l.grad_dest, sizeof(double) * nb * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_expected_fit(cpm_ctx *c, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const double *pi0, uint32_t flags,
                         const double *weights, double *record, double *expected, double *cotangent, double *grad_p_drive, double *grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if ((rc = fit_check(c, "expected_fit", B, p_min, p_max, e_drive, flags, weights, record)) != CPM_OK) return rc;
    if (grad_dest && !(flags & CPM_FIT_DEST)) return fail(CPM_ERR_ARG, "expected_fit: grad_dest without CPM_FIT_DEST");
    return expected_fit_blocking(c, B, p_min, p_max, e_drive, pi0, flags, weights, record, expected, cotangent, grad_p_drive, grad_dest, false);
}

// ... from the compact rows (include/cpm_expected_sparse_grad.h): the e_dest direction needs the compact tangent of
// include/cpm_expected_sparse_dest.h; the dense one is never read
static int32_t fit_sparse_check(cpm_ctx *c, const char *what, int32_t B, const double *p_min, const double *p_max, const double *e_drive, uint32_t flags,
                         const double *weights, const void *record, const void *grad_dest)
{
    if ((flags & CPM_FIT_DEST) && !(c->sdp_valid && c->d_sdp))
        return fail(CPM_ERR_ARG, "%s: CPM_FIT_DEST: the p_destin tangent is a dense [T][Z][Z] array, which the sparse calls never read (cpm_expected_fit); "
                                 "install a compact one with cpm_build_p_dest_tangent_sparse or cpm_set_p_dest_tangent_sparse",
                    what);
    int32_t rc = fit_check(c, what, B, p_min, p_max, e_drive, flags, weights, record, true);
    if (rc != CPM_OK) return rc;
    if (grad_dest && !(flags & CPM_FIT_DEST)) return fail(CPM_ERR_ARG, "%s: grad_dest without CPM_FIT_DEST", what);
    return exps_rows_ready(c, what);
}

int32_t cpm_expected_sparse_fit_dev(cpm_ctx *c, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const void *d_pi0, uint32_t flags,
                                    const double *weights, void *d_record, void *d_expected, void *d_cotangent, void *d_grad_p_drive, void *d_grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if ((rc = fit_sparse_check(c, "expected_sparse_fit_dev", B, p_min, p_max, e_drive, flags, weights, d_record, d_grad_dest)) != CPM_OK) return rc;
    return expected_fit_enqueue(c, B, p_min, p_max, e_drive, static_cast<const double *>(d_pi0), flags, weights, static_cast<double *>(d_record),
                                static_cast<double *>(d_expected), static_cast<double *>(d_cotangent), static_cast<double *>(d_grad_p_drive),
                                static_cast<double *>(d_grad_dest), true);
}

int32_t cpm_expected_sparse_fit(cpm_ctx *c, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const double *pi0, uint32_t flags,
                                const double *weights, double *record, double *expected, double *cotangent, double *grad_p_drive, double *grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if ((rc = fit_sparse_check(c, "expected_sparse_fit", B, p_min, p_max, e_drive, flags, weights, record, grad_dest)) != CPM_OK) return rc;
    return expected_fit_blocking(c, B, p_min, p_max, e_drive, pi0, flags, weights, record, expected, cotangent, grad_p_drive, grad_dest, true);
}

// ------------------------------------------------------------------ the e_dest direction from a compact tangent (include/cpm_expected_sparse_dest.h)
// what the three calls that install or read the compact tangent need: tables with compact rows, and the table itself
static int32_t sdp_reserve(cpm_ctx *c, const char *what)
{
    int32_t rc = exps_rows_ready(c, what);
    if (rc != CPM_OK) return rc;
    HIP_TRY(c->d_sdp.reserve(static_cast<size_t>(c->T) * c->Z * cpm::kDsCap));
    return CPM_OK;
}

int32_t cpm_build_p_dest_tangent_sparse(cpm_ctx *c)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    CTX_TRY(c);
    if (!c->have_cdf || !c->dest_built)
        return fail(CPM_ERR_STATE, "build_p_dest_tangent_sparse: the installed p_destin tables do not come from cpm_build_p_dest on the resident datamatrix");
    if (!c->have_dmat) return fail(CPM_ERR_STATE, "build_p_dest_tangent_sparse: no datamatrix is resident");
    if (!(c->dest_built_e > 0.0))
        return fail(CPM_ERR_STATE, "build_p_dest_tangent_sparse: the tables were built with e_dest = %g; the tangent needs e_dest > 0", c->dest_built_e);
    if (!c->sparse_tables) return exps_no_rows();
    if (c->tables_uploaded || !c->ds_valid || !c->ds_ok)
        return fail(CPM_ERR_STATE, "build_p_dest_tangent_sparse: the compact rows these tables were built from are gone");
    c->sdp_valid = false;
    if ((rc = sdp_reserve(c, "build_p_dest_tangent_sparse")) != CPM_OK) return rc;
    const int64_t rows = c->T * c->Z;
    cpm::launch(cpm::k_exps_tan_cells, dim3(nblk(rows, 64)), dim3(64), 0, c->stream, c->d_ds_cells.get(), c->d_sp.get(), c->d_sj.get(), c->d_scnt.get(),
                cpm::kDsCap, rows, static_cast<int>(c->Z), c->d_sdp.get());
    HIP_TRY(hipGetLastError());
    c->sdp_valid = true;
    ++c->sdp_gen;
    return CPM_OK;
}

int32_t cpm_set_p_dest_tangent_sparse(cpm_ctx *c, const double *dp)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!dp) return fail(CPM_ERR_ARG, "set_p_dest_tangent_sparse: null dp");
    CTX_TRY(c);
    if ((rc = exps_rows_ready(c, "set_p_dest_tangent_sparse")) != CPM_OK) return rc;
    const size_t Z = static_cast<size_t>(c->Z), T = static_cast<size_t>(c->T), block = Z * Z;
    for (size_t i = 0; i < block * T; ++i)
        if (!std::isfinite(dp[i]))
            return fail(CPM_ERR_ARG, "set_p_dest_tangent_sparse: the entry of origin %lld, destination %lld, hour %lld is not finite", (long long)(i % Z) + 1,
                        (long long)(i / Z % Z) + 1, (long long)(i / block) + 1);
    // first every hour is checked against the stored cells, then every hour is moved: a refused array leaves the installed tangent alone
    HIP_TRY(c->d_sdp_stage.reserve(block));
    HIP_TRY(c->d_sdp_bad.reserve(1));
    HIP_TRY(c->h_sdp_bad.reserve(1));
    HIP_TRY(hipMemsetAsync(c->d_sdp_bad, 0xff, sizeof(unsigned long long), c->stream));
    const int Zi = static_cast<int>(Z);
    for (size_t t = 0; t < T; ++t) {
        HIP_TRY(hipMemcpyAsync(c->d_sdp_stage, dp + t * block, sizeof(double) * block, hipMemcpyHostToDevice, c->stream));
        cpm::launch(cpm::k_exps_tan_check, dim3(nblk(c->Z, 256), static_cast<unsigned>(Z)), dim3(256), 0, c->stream,
                    static_cast<const double *>(c->d_sdp_stage.get()), static_cast<const uint32_t *>(c->d_sj + t * Z * cpm::kDsCap),
                    static_cast<const uint32_t *>(c->d_scnt + t * Z), cpm::kDsCap, Zi, static_cast<unsigned long long>(t * block), c->d_sdp_bad.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(c->h_sdp_bad, c->d_sdp_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const unsigned long long bad = *c->h_sdp_bad;
    if (bad != ~0ull) {
        c->d_sdp_stage.release();
        return fail(CPM_ERR_TABLE, "set_p_dest_tangent_sparse: the entry of hour %llu, origin %llu, destination %llu is not zero, but the compact rows do not "
                                   "store that cell",
                    bad / block + 1, bad % Z + 1, bad / Z % Z + 1);
    }
    c->sdp_valid = false;
    if ((rc = sdp_reserve(c, "set_p_dest_tangent_sparse")) != CPM_OK) return rc;
    for (size_t t = 0; t < T; ++t) {
        HIP_TRY(hipMemcpyAsync(c->d_sdp_stage, dp + t * block, sizeof(double) * block, hipMemcpyHostToDevice, c->stream));
        cpm::launch(cpm::k_exps_tan_gather, dim3(nblk(cpm::kDsCap, 64), static_cast<unsigned>(Z)), dim3(64), 0, c->stream,
                    static_cast<const double *>(c->d_sdp_stage.get()), static_cast<const uint32_t *>(c->d_sj + t * Z * cpm::kDsCap),
                    static_cast<const uint32_t *>(c->d_scnt + t * Z), cpm::kDsCap, Zi, c->d_sdp + t * Z * cpm::kDsCap);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_sdp_stage.release();
    c->sdp_valid = true;
    ++c->sdp_gen;
    return CPM_OK;
}

int32_t cpm_get_p_dest_tangent_sparse(cpm_ctx *c, double *out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!out) return fail(CPM_ERR_ARG, "get_p_dest_tangent_sparse: null out");
    CTX_TRY(c);
    if ((rc = exps_rows_ready(c, "get_p_dest_tangent_sparse")) != CPM_OK) return rc;
    if ((rc = sdp_ready(c, "get_p_dest_tangent_sparse")) != CPM_OK) return rc;
    const size_t Z = static_cast<size_t>(c->Z), T = static_cast<size_t>(c->T), block = Z * Z;
    HIP_TRY(c->d_sdp_stage.reserve(block));
    for (size_t t = 0; t < T; ++t) {
        HIP_TRY(hipMemsetAsync(c->d_sdp_stage, 0, sizeof(double) * block, c->stream));
        cpm::launch(cpm::k_exps_tan_scatter, dim3(nblk(cpm::kDsCap, 64), static_cast<unsigned>(Z)), dim3(64), 0, c->stream,
                    static_cast<const double *>(c->d_sdp + t * Z * cpm::kDsCap), static_cast<const uint32_t *>(c->d_sj + t * Z * cpm::kDsCap),
                    static_cast<const uint32_t *>(c->d_scnt + t * Z), cpm::kDsCap, static_cast<int>(Z), c->d_sdp_stage.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + t * block, c->d_sdp_stage, sizeof(double) * block, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_sdp_stage.release();
    return CPM_OK;
}

int32_t cpm_expected_sparse_grad_dest_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext, void *d_grad_p_drive,
                                          void *d_grad_pi0, void *d_grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest_dev: null d_cotangent");
    if (!d_grad_p_drive || !d_grad_dest) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest_dev: null d_grad_p_drive or d_grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;
    return expected_grad_dest_enqueue(c, static_cast<const double *>(d_pi0), flags, static_cast<const double *>(d_cotangent),
                                      static_cast<const double *>(d_gnext), static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0),
                                      static_cast<double *>(d_grad_dest), true);
}

int32_t cpm_expected_sparse_grad_dest(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving, const double *g_next,
                                      double *grad_p_drive, double *grad_pi0, double *grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest: null cotangents");
    if (!grad_p_drive || !grad_dest) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest: null grad_p_drive or grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, false, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;  // (state is refused before a cotangent is read or copied)
    if ((rc = sdp_ready(c, "expected_sparse_grad_dest")) != CPM_OK) return rc;
    return expected_grad_dest_blocking(c, pi0, flags, g_parking, g_driving, g_next, grad_p_drive, grad_pi0, grad_dest, true);
}

int32_t cpm_expected_sparse_grad_dest_batch_dev(cpm_ctx *c, const void *d_pi0, uint32_t flags, const void *d_cotangent, const void *d_gnext,
                                                void *d_grad_p_drive, void *d_grad_pi0, void *d_grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_cotangent) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest_batch_dev: null d_cotangent");
    if (!d_grad_p_drive || !d_grad_dest) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest_batch_dev: null d_grad_p_drive or d_grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;
    return expected_grad_batch_enqueue(c, static_cast<const double *>(d_pi0), flags, tb.B, tb.pd, tb.q_stride, static_cast<const double *>(d_cotangent),
                                       static_cast<const double *>(d_gnext), static_cast<double *>(d_grad_p_drive), static_cast<double *>(d_grad_pi0),
                                       static_cast<double *>(d_grad_dest), true);
}

int32_t cpm_expected_sparse_grad_dest_batch(cpm_ctx *c, const double *pi0, uint32_t flags, const double *g_parking, const double *g_driving,
                                            const double *g_next, double *grad_p_drive, double *grad_pi0, double *grad_dest)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!g_parking || !g_driving) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest_batch: null cotangents");
    if (!grad_p_drive || !grad_dest) return fail(CPM_ERR_ARG, "expected_sparse_grad_dest_batch: null grad_p_drive or grad_dest");
    ExpTables tb;
    if ((rc = exp_tables(c, flags, true, tb)) != CPM_OK) return rc;
    if ((rc = exps_rows_ready(c, "expected")) != CPM_OK) return rc;  // (state is refused before a cotangent is read or copied)
    if ((rc = sdp_ready(c, "expected_sparse_grad_dest_batch")) != CPM_OK) return rc;
    return expected_grad_batch_blocking(c, "expected_sparse_grad_dest_batch", pi0, flags, tb.B, tb.pd, tb.q_stride, g_parking, g_driving, g_next, grad_p_drive,
                                        grad_pi0, grad_dest, true);
}

int32_t cpm_expected_sparse_trip_tangent_dev(cpm_ctx *c, void *d_dw)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_dw) return fail(CPM_ERR_ARG, "expected_sparse_trip_tangent_dev: null d_dw");
    CTX_TRY(c);
    return trip_tangent_sparse_enqueue(c, static_cast<double *>(d_dw));
}

int32_t cpm_expected_sparse_trip_tangent(cpm_ctx *c, double *dw_sec, double *dw_km)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!dw_sec || !dw_km) return fail(CPM_ERR_ARG, "expected_sparse_trip_tangent: null outputs");
    CTX_TRY(c);
    const size_t zt = static_cast<size_t>(c->Z) * c->T;
    HIP_TRY(c->d_tan_w.reserve(2 * zt));
    if ((rc = trip_tangent_sparse_enqueue(c, c->d_tan_w)) != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dw_sec, c->d_tan_w, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dw_km, c->d_tan_w + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ forward tangent of the expected densities (include/cpm_expected_tangent.h)

// both forms for both table layouts (what: the entry's name in its error texts)
static int32_t expected_tangent_dev_any(cpm_ctx *c, const char *what, bool sparse, int32_t K, const void *d_pi0, uint32_t flags, const void *d_dpi0,
                                        const void *d_dp_drive, const double *c_dest, void *d_out, void *d_dpi_next, void *d_expected)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if ((rc = tangent_check(c, what, K, flags, c_dest, d_out, sparse)) != CPM_OK) return rc;
    return expected_tangent_enqueue(c, K, static_cast<const double *>(d_pi0), flags, static_cast<const double *>(d_dpi0),
                                    static_cast<const double *>(d_dp_drive), c_dest, static_cast<double *>(d_out), static_cast<double *>(d_dpi_next),
                                    static_cast<double *>(d_expected), sparse);
}

static int32_t expected_tangent_any(cpm_ctx *c, const char *what, bool sparse, int32_t K, const double *pi0, uint32_t flags, const double *dpi0,
                                    const double *dp_drive, const double *c_dest, double *d_parking, double *d_driving, double *dpi_next, double *parking,
                                    double *driving)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if ((rc = tangent_check(c, what, K, flags, c_dest, d_parking, sparse)) != CPM_OK) return rc;
    if (!d_driving) return fail(CPM_ERR_ARG, "%s: null tangent output", what);
    if ((parking == nullptr) != (driving == nullptr)) return fail(CPM_ERR_ARG, "%s: parking and driving go together", what);
    if ((rc = check_pi0(c, pi0)) != CPM_OK) return rc;
    const size_t Z = static_cast<size_t>(c->Z), zt = Z * static_cast<size_t>(c->T), nk = static_cast<size_t>(K);
    if ((rc = check_finite(what, "dpi0", dpi0, nk * Z)) != CPM_OK) return rc;
    if ((rc = check_finite(what, "dp_drive", dp_drive, nk * zt)) != CPM_OK) return rc;
    if ((rc = sparse ? ensure_exps(c) : ensure_exp_aux(c)) != CPM_OK) return rc;  // (the row-total check: CPM_ERR_TABLE in front of the first copy)
    // [K][2][T][Z] out | [2][T][Z] primal | [K][Z] d pi_next | [Z] pi_0 | [K][Z] d pi_0 | [K][T][Z] d p_drive
    HIP_TRY(c->d_tanf_io.reserve(nk * 2 * zt + 2 * zt + nk * Z + Z + nk * Z + nk * zt));
    double *d_out = c->d_tanf_io, *d_exp = d_out + nk * 2 * zt, *d_next = d_exp + 2 * zt, *d_pi0 = d_next + nk * Z, *d_dpi0 = d_pi0 + Z,
           *d_dpd = d_dpi0 + nk * Z;
    if (pi0) HIP_TRY(hipMemcpyAsync(d_pi0, pi0, sizeof(double) * Z, hipMemcpyHostToDevice, c->stream));
    if (dpi0) HIP_TRY(hipMemcpyAsync(d_dpi0, dpi0, sizeof(double) * nk * Z, hipMemcpyHostToDevice, c->stream));
    if (dp_drive) HIP_TRY(hipMemcpyAsync(d_dpd, dp_drive, sizeof(double) * nk * zt, hipMemcpyHostToDevice, c->stream));
    rc = expected_tangent_enqueue(c, K, pi0 ? d_pi0 : nullptr, flags, dpi0 ? d_dpi0 : nullptr, dp_drive ? d_dpd : nullptr, c_dest, d_out,
                                  dpi_next ? d_next : nullptr, parking ? d_exp : nullptr, sparse);
    if (rc != CPM_OK) return rc;
    for (size_t k = 0; k < nk; ++k) {
        HIP_TRY(hipMemcpyAsync(d_parking + k * zt, d_out + k * 2 * zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(d_driving + k * zt, d_out + k * 2 * zt + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    }
    if (dpi_next) HIP_TRY(hipMemcpyAsync(dpi_next, d_next, sizeof(double) * nk * Z, hipMemcpyDeviceToHost, c->stream));
    if (parking) {
        HIP_TRY(hipMemcpyAsync(parking, d_exp, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(driving, d_exp + zt, sizeof(double) * zt, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_expected_tangent_dev(cpm_ctx *c, int32_t K, const void *d_pi0, uint32_t flags, const void *d_dpi0, const void *d_dp_drive, const double *c_dest,
                                 void *d_out, void *d_dpi_next, void *d_expected)
{
    return expected_tangent_dev_any(c, "expected_tangent_dev", false, K, d_pi0, flags, d_dpi0, d_dp_drive, c_dest, d_out, d_dpi_next, d_expected);
}

int32_t cpm_expected_tangent(cpm_ctx *c, int32_t K, const double *pi0, uint32_t flags, const double *dpi0, const double *dp_drive, const double *c_dest,
                             double *d_parking, double *d_driving, double *dpi_next, double *parking, double *driving)
{
    return expected_tangent_any(c, "expected_tangent", false, K, pi0, flags, dpi0, dp_drive, c_dest, d_parking, d_driving, dpi_next, parking, driving);
}

// ... from the compact rows and the compact tangent (include/cpm_expected_sparse_tangent.h)
int32_t cpm_expected_sparse_tangent_dev(cpm_ctx *c, int32_t K, const void *d_pi0, uint32_t flags, const void *d_dpi0, const void *d_dp_drive,
                                        const double *c_dest, void *d_out, void *d_dpi_next, void *d_expected)
{
    return expected_tangent_dev_any(c, "expected_sparse_tangent_dev", true, K, d_pi0, flags, d_dpi0, d_dp_drive, c_dest, d_out, d_dpi_next, d_expected);
}

int32_t cpm_expected_sparse_tangent(cpm_ctx *c, int32_t K, const double *pi0, uint32_t flags, const double *dpi0, const double *dp_drive, const double *c_dest,
                                    double *d_parking, double *d_driving, double *dpi_next, double *parking, double *driving)
{
    return expected_tangent_any(c, "expected_sparse_tangent", true, K, pi0, flags, dpi0, dp_drive, c_dest, d_parking, d_driving, dpi_next, parking, driving);
}

int32_t cpm_build_p_drive_tangent_dev(cpm_ctx *c, double p_min, double p_max, double e_drive, void *d_out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!d_out) return fail(CPM_ERR_ARG, "build_p_drive_tangent_dev: null d_out");
    CTX_TRY(c);
    return pdrive_tangent_enqueue(c, p_min, p_max, e_drive, static_cast<double *>(d_out));
}

int32_t cpm_build_p_drive_tangent(cpm_ctx *c, double p_min, double p_max, double e_drive, double *out)
{
    int32_t rc = exp_enter(c);
    if (rc != CPM_OK) return rc;
    if (!out) return fail(CPM_ERR_ARG, "build_p_drive_tangent: null out");
    CTX_TRY(c);
    const size_t words = 3 * static_cast<size_t>(c->Z) * c->T;
    HIP_TRY(c->d_tanf_io.reserve(words));
    if ((rc = pdrive_tangent_enqueue(c, p_min, p_max, e_drive, c->d_tanf_io)) != CPM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_tanf_io, sizeof(double) * words, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

// ------------------------------------------------------------------ batch (include/cpm_batch.h)

int32_t cpm_set_p_drive_batch(cpm_ctx *c, int32_t B, const double *p_drives)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");
    if (B < 1 || B > CPM_MAX_BATCH) return fail(CPM_ERR_ARG, "set_p_drive_batch: B = %d outside 1..%d", B, CPM_MAX_BATCH);
    if (!p_drives) return fail(CPM_ERR_ARG, "set_p_drive_batch: null p_drives");
    CTX_TRY(c);
    int32_t rc = ensure_batch_tables(c, B);
    if (rc != CPM_OK) return rc;
    const int64_t cells = static_cast<int64_t>(B) * c->T * c->Z;
    HIP_TRY(hipMemcpyAsync(c->d_pdrive_b, p_drives, sizeof(double) * cells, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cpm::k_build_thr, dim3(nblk(cells, 256)), dim3(256), 0, c->stream, c->d_pdrive_b, c->d_thr_b, cells);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->batch_B = B;
    return CPM_OK;
}

int32_t cpm_build_p_drive_batch(cpm_ctx *c, int32_t B, const double *p_min, const double *p_max, const double *e_drive)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");
    if (B < 1 || B > CPM_MAX_BATCH) return fail(CPM_ERR_ARG, "build_p_drive_batch: B = %d outside 1..%d", B, CPM_MAX_BATCH);
    if (!p_min || !p_max || !e_drive) return fail(CPM_ERR_ARG, "build_p_drive_batch: null parameter array");
    CTX_TRY(c);
    if (!c->have_dm()) return fail(CPM_ERR_STATE, "build_p_drive_batch: datamatrix and distance matrix first");
    int32_t rc = ensure_batch_tables(c, B);
    if (rc == CPM_OK) rc = ensure_pdrive_mean(c);
    if (rc != CPM_OK) return rc;
    const size_t zt = static_cast<size_t>(c->Z * c->T);
    for (int b = 0; b < B; ++b)  // (the kernel of cpm_build_p_drive: the same table bit for bit; the call returns once they are enqueued)
        hipLaunchKernelGGL(cpm::k_pdrive_final, dim3(nblk(c->Z, 64), static_cast<unsigned>(c->T)), dim3(64), 0, c->stream, c->d_pdrive_mean,
                           c->d_pdrive_b + b * zt, c->d_thr_b + b * zt, static_cast<int>(c->Z), static_cast<int>(c->T), p_min[b], p_max[b], e_drive[b]);
    HIP_TRY(hipGetLastError());
    c->batch_B = B;
    return CPM_OK;
}

int32_t cpm_get_p_drive_batch(cpm_ctx *c, double *out)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");
    if (!out) return fail(CPM_ERR_ARG, "get_p_drive_batch: null out");
    CTX_TRY(c);
    if (c->batch_B < 1) return fail(CPM_ERR_STATE, "get_p_drive_batch: no batch tables");
    HIP_TRY(hipMemcpyAsync(out, c->d_pdrive_b, sizeof(double) * c->batch_B * c->Z * c->T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CPM_OK;
}

int32_t cpm_resample_batch(cpm_ctx *c, const uint64_t *seeds, uint32_t flags, int64_t *parking, int64_t *driving, int64_t *sum_tt_q16)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");
    if (!parking || !driving) return fail(CPM_ERR_ARG, "resample_batch: null count outputs");
    CTX_TRY(c);
    int32_t rc = batch_ready(c, seeds, flags);
    if (rc != CPM_OK) return rc;
    absorb_batch_status(c);
    const int B = c->batch_B;
    const size_t zt = static_cast<size_t>(c->Z * c->T), nwords = 2 * zt + 2;
    FleetTable fleet(c);
    fleet.use(0);
    auto single = [&](int b) -> int32_t {  // fleet b through the single-fleet step (its own repeats and fallbacks included)
        fleet.use(b);
        int32_t r = resample_blocking(c, seeds[b], flags);
        if (r != CPM_OK) return r;
        copy_counts(c, parking, driving, sum_tt_q16, b);
        return CPM_OK;
    };
    if (!batch_grouped(c)) {  // the grouped path would not run this problem: every fleet with the context's kernel choice
        for (int b = 0; b < B && rc == CPM_OK; ++b) rc = single(b);
        return rc;
    }
    HIP_TRY(c->d_bcounts.reserve(nwords * B));
    HIP_TRY(c->h_bcounts.reserve(nwords * B));
    std::vector<int32_t> todo(B);
    for (int b = 0; b < B; ++b) todo[b] = b;
    std::vector<char> by_single(B, 0);
    int batched = B;
    for (;;) {
        std::vector<uint64_t> sd(todo.size());
        for (size_t k = 0; k < todo.size(); ++k) sd[k] = seeds[todo[k]];
        rc = batch_enqueue(c, sd, todo, todo, flags, c->d_bcounts);
        if (rc != CPM_OK) return rc;
        for (int32_t b : todo)
            HIP_TRY(hipMemcpyAsync(c->h_bcounts + b * nwords, c->d_bcounts + b * nwords, sizeof(int64_t) * nwords, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::vector<int32_t> over;
        for (int32_t b : todo)
            if (c->h_bcounts[b * nwords + nwords - 1] != 0) over.push_back(b);
        if (over.empty()) break;
        // a bucket or a run of these fleets outgrew its region: again, those fleets only, with twice the batch's regions while the
        // problem still fits ...  (each discarded attempt: CPM_INFO_STEPS_REPEATED)
        ++c->steps_repeated;
        if (grow_batch(c)) {
            todo = over;
            continue;
        }
        for (int32_t b : over) {  // ... else one at a time through the single-fleet step
            rc = single(b);
            if (rc != CPM_OK) return rc;
            by_single[b] = 1;
            --batched;
        }
        break;
    }
    for (int b = 0; b < B; ++b) {
        if (by_single[b]) continue;
        copy_counts(c, parking, driving, sum_tt_q16, b, c->h_bcounts + b * nwords);
    }
    c->last_batch_fleets = batched;
    if (batched > 0) {
        c->last_kernel = CPM_KERNEL_ZONE_GROUPED;
        c->last_form = CPM_FORM_BATCH;
        c->last_hour = c->zb.last_hour_counted;
        c->last_cells = c->zb.last_cells;
    }
    return CPM_OK;
}

int32_t cpm_resample_batch_dev(cpm_ctx *c, const uint64_t *seeds, uint32_t flags, void *d_counts)
{
    if (!c) return fail(CPM_ERR_ARG, "null context");
    if (!d_counts) return fail(CPM_ERR_ARG, "resample_batch_dev: null d_counts");
    CTX_TRY(c);
    int32_t rc = batch_ready(c, seeds, flags);
    if (rc != CPM_OK) return rc;
    absorb_batch_status(c);
    const int B = c->batch_B;
    const size_t nwords = static_cast<size_t>(2 * c->T * c->Z + 2);
    int64_t *counts = static_cast<int64_t *>(d_counts);
    FleetTable fleet(c);
    fleet.use(0);
    if (!batch_grouped(c)) {
        for (int b = 0; b < B && rc == CPM_OK; ++b) {
            fleet.use(b);
            rc = resample_enqueue(c, seeds[b], flags, counts + b * nwords);
        }
        return rc;
    }
    std::vector<int32_t> all(B);
    for (int b = 0; b < B; ++b) all[b] = b;
    rc = batch_enqueue(c, std::vector<uint64_t>(seeds, seeds + B), all, all, flags, counts);
    if (rc != CPM_OK) return rc;
    if (!c->bstatus_pending) {  // (one step's status in flight at a time: a later one is looked at when that one has been)
        HIP_TRY(c->d_bstatus.reserve(1));
        HIP_TRY(c->h_bstatus.reserve(1));
        if (!c->bstatus_ev) HIP_TRY(hipEventCreateWithFlags(&c->bstatus_ev, hipEventDisableTiming));
        hipLaunchKernelGGL(cpm::k_batch_status, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<const unsigned long long *>(counts), nwords, B, c->d_bstatus);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_bstatus, c->d_bstatus, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->bstatus_ev, c->stream));
        c->bstatus_pending = true;
    }
    c->last_batch_fleets = B;
    c->last_kernel = CPM_KERNEL_ZONE_GROUPED;
    c->last_form = CPM_FORM_BATCH;
    c->last_hour = c->zb.last_hour_counted;
    c->last_cells = c->zb.last_cells;
    return CPM_OK;
}

#ifdef CPM_DIAGNOSTIC
// diagnostic builds only (tools/place_stamps.py): a side buffer for the s_memtime stamps of the placing kernel; n_blocks x 8 words
int32_t cpm_diag_place_stamps(cpm_ctx *c, unsigned long long *host_out_or_null, int64_t n_blocks)
{
    CTX_TRY(c);
    static unsigned long long *d_buf = nullptr;
    static int64_t cap = 0;
    if (!host_out_or_null) {  // arm
        if (cap < n_blocks) {
            if (d_buf) (void)hipFree(d_buf);
            HIP_TRY(hipMalloc(&d_buf, sizeof(unsigned long long) * 8 * n_blocks));
            cap = n_blocks;
        }
        HIP_TRY(hipMemset(d_buf, 0, sizeof(unsigned long long) * 8 * n_blocks));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(cpm::g_place_stamps), &d_buf, sizeof(d_buf)));
        return CPM_OK;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host_out_or_null, d_buf, sizeof(unsigned long long) * 8 * std::min(n_blocks, cap), hipMemcpyDeviceToHost));
    return CPM_OK;
}
#endif

}  // extern "C"
