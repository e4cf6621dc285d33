/*
 * cpm_charge.h -- EV state of charge, hourly charging load per zone and uncovered trips from the fused resample of libcpm_hip.so.
 *
 * cpm_resample says where cars stand, cpm_flows.h where they go, cpm_stays.h how long they stay, cpm_paths.h what each car did.  The
 * calls below answer what a parking map is drawn for: how much energy is drawn from chargers in which zone in which hour, and which
 * trips the battery could not cover -- the reference's own first extension (README 4: "the states of charge of electric car
 * batteries", "fuel consumption ... for each trip").  A car's charge is a recurrence over its whole day and the driven distance of a
 * trip is drawn per driver, so neither a host loop nor the per-car record gets there without 32 bytes per car-hour of f64 matrices.
 *
 * Definition.  Hours are 0-based: t = 0 .. T-1 is the reference's hour t+1.  n is the context's car count.
 *   Parameters (cpm_charge_params):
 *     capacity_wh    uint32   battery capacity in Wh: >= 1, else CPM_ERR_ARG
 *     power_wh       uint32   Wh a parked car takes per hour, where zone_power_wh is NULL
 *     initial_wh     uint32   every car's charge at hour 0, where soc_in is NULL: <= capacity_wh, else CPM_ERR_ARG
 *     wh_per_km      f64      energy per km driven: finite and >= 0, else CPM_ERR_ARG
 *     zone_power_wh  uint32[Z] or NULL   charger power per zone; 0 = no charger in the zone
 *     soc_in         uint32[n] or NULL   initial charge per local car; values above capacity_wh are clamped to it
 *     The array fields are host pointers in the blocking call and device pointers in the _dev call.
 *   Recurrence.  Car i starts with E = soc_in ? min(soc_in[i], capacity_wh) : initial_wh.  For t = 0 .. T-1, with
 *     z = state_matrix[i,t] - 1:
 *     The car drove (transition_matrix[i,t,1] == 1):
 *       d = transition_matrix[i,t,4] exactly as cpm_resample(..., trans_out) returns it under CPM_FLAG_TRAVEL: 1.0 km for a trip
 *         inside a zone; otherwise the truncated-normal draw of Philox stream 2 at step T-1+t, keyed by the GLOBAL car id, mean
 *         dist[o,d], sigma a tenth of it.
 *       u = rint(d * wh_per_km): one f64 multiply, round half to even (the library is built -ffp-contract=off).
 *       If !(u >= 0) then u = 0 (a NaN distance costs nothing).
 *       If u > E: short[z][t] += 1 and drawn = E.  Else drawn = u.
 *       used[z][t] += drawn, E -= drawn.
 *       The car does not charge in an hour it drives in.
 *     The car is parked: give = min(P_z, capacity_wh - E), charge[z][t] += give, E += give.
 *       P_z = zone_power_wh ? zone_power_wh[z] : power_wh.
 *     Hour T-1 is sampled and not applied (src/resampling.jl:81-83).  It counts here as it does in cpm_flows.h and cpm_stays.h: a car
 *       that drives in it spends the energy, a car that does not drive charges.
 *     soc_out[i] = E after hour T-1.
 *   Outputs.
 *     charge       int64[Z][T]   Wh delivered by the chargers of zone z+1 in hour t: the charging load map.
 *     used         int64[Z][T]   Wh taken from batteries by trips that START in zone z+1 in hour t.
 *     short_trips  int32[Z][T]   trips from z+1 in hour t that the battery did not cover.
 *     soc_out      uint32[n]     may be NULL.
 *     charge, used and short_trips are row-major, zone-major, like `parked` of cpm_stays.h.  The call writes every word of every
 *     array it is given.
 *   Identities.  sum_i E_i(0) + sum charge - sum used == sum soc_out.  short_trips[z][t] <= driving[z][t].
 *     charge[z][t] <= P_z * (parking[z][t] - driving[z][t]).
 *   Sharding.  charge, used and short_trips of the shards of a fleet add exactly.  soc_out rows are disjoint.
 *   Limits.  T <= 255 and Z < 2^24, as in cpm_stays.h: the hour of the last drive is kept in 8 bits.  Beyond them: CPM_ERR_ARG.
 *   Distance matrix.  The calls need a resident distance matrix, by whatever route made one resident (cpm_set_datamatrix with dist,
 *     cpm_set_distance, cpm_set_distance_from_centroids).  Without one they give CPM_ERR_STATE with a message.  They do NOT need a
 *     datamatrix or CPM_FLAG_TRAVEL.  The flag may be combined, and then only adds the travel-time sum as it does everywhere.  The
 *     arrays do not depend on it.
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, no CPU fallback.
 */
#ifndef CPM_CHARGE_H
#define CPM_CHARGE_H

#include "cpm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cpm_charge_params {
    uint32_t capacity_wh;
    uint32_t power_wh;
    uint32_t initial_wh;
    double wh_per_km;
    const uint32_t *zone_power_wh;
    const uint32_t *soc_in;
} cpm_charge_params;

/* resampling (src/resampling.jl:3-89) as cpm_resample returns it, plus the arrays defined above.  Blocking.
 * flags as for cpm_resample; parking, driving and the travel-time sum are bit for bit those of cpm_resample with the same seed and
 * flags; the context's state is left unchanged; an overflowed step is repaired by the call itself, and the arrays returned are those
 * of the attempt whose counts are returned.  charge_out, used_out: int64[Z*T]; short_out: int32[Z*T]; soc_out: uint32[n] or NULL.
 * NULL params, charge_out, used_out or short_out: CPM_ERR_ARG.  sum_travel_time_q16 may be NULL. */
int32_t cpm_resample_charge(cpm_ctx *ctx, uint64_t seed, uint32_t flags, const cpm_charge_params *params, int64_t *parking_counts,
                            int64_t *driving_counts, int64_t *sum_travel_time_q16, int64_t *charge_out, int64_t *used_out,
                            int32_t *short_out, uint32_t *soc_out);
/* device-resident form, enqueued on the context's stream with no synchronisation: d_counts as for cpm_resample_dev; d_charge, d_used
 * DEVICE int64[Z*T], d_short DEVICE int32[Z*T], d_soc DEVICE uint32[n] or NULL; the array fields of params are DEVICE pointers and
 * must stay valid until the step has run.  status != 0 in d_counts invalidates all four arrays; the caller repeats the step.  Nothing
 * is ever stored outside the caller's arrays, also in an overflowed attempt. */
int32_t cpm_resample_charge_dev(cpm_ctx *ctx, uint64_t seed, uint32_t flags, const cpm_charge_params *params, void *d_counts,
                                void *d_charge, void *d_used, void *d_short, void *d_soc);

#ifdef __cplusplus
}
#endif
#endif
