// cpm_objectives.h -- the sweep's objectives from a count tensor on the device (include/cpm_objectives.h): k_measured_flag, k_obj_zones,
// k_obj_final.
//
// A count tensor is parking[T][Z] | driving[T][Z] | sum_tt_q16 | status, Z contiguous.  k_obj_zones gives a zone to a thread and 256
// consecutive zones of one fleet to a workgroup (grid = (ceil(Z/256), B)): an hour's loads of a wave are 64 consecutive int64 words.
// Pass 1 walks the hours once for the zone's integer extremes and the hour sums -- a wave reduction, then ONE int64 atomic per wave,
// hour and tensor half into the record (integer sums are order-free and exact; the build switches the compiler's atomic optimizer
// off, so the aggregation is done here as in the other kernels).  Pass 2 walks them again (the tensor is in L2 by then) for the
// zone's error: the operations of include/cpm_objectives.h, one IEEE f64 operation each, in that order.
//
// The zone sum takes no floating-point atomics.  A workgroup adds its 256 errors (0.0 for a zone that is not valid: adding +0.0 to a
// sum of non-negative terms changes no bit) through the fixed tree of a wave reduction and its four waves in order, and leaves the
// partial and its count of valid zones in the context's workspace; k_obj_final (grid = B, one wave) adds a fleet's partials -- lane l
// takes partials l, l + 64, ... in order, then the same tree -- and writes words 0..3.  The order depends on Z alone.  No spinning,
// no last-block ticket: the second launch is the ordering.
//
// Separate kernels in a header of their own: the hourly kernels' code does not move.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cpm {

constexpr int kObjBlock = 256;
constexpr int kObjHead = 4;  // words of a record in front of the hour sums

// flag[z] = the zone's measured row, added in hour order, is != 0 (README.md:2236).  measured is [T][Z].
__global__ __launch_bounds__(kObjBlock) void k_measured_flag(const double *__restrict__ measured, int *__restrict__ flag, int Z, int T)
{
    const int z = static_cast<int>(blockIdx.x) * kObjBlock + static_cast<int>(threadIdx.x);
    if (z >= Z) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s = s + measured[static_cast<size_t>(t) * Z + z];
    flag[z] = (s != 0.0) ? 1 : 0;
}

// the fixed tree of a wave: lane 0 ends with ((..) + (..)) of all 64 lanes, the same pairing every time
__device__ __forceinline__ double obj_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
    return v;
}

// grid = (ceil(Z/256), B).  obj is zeroed by the caller.  measured / flag: nullptr when no measured data is installed.
// part: [B][gridDim.x] f64, part_n: [B][gridDim.x] int.  Every thread stays until the end (the wave reductions take all lanes).
__global__ __launch_bounds__(kObjBlock) void k_obj_zones(const long long *__restrict__ counts, const double *__restrict__ measured,
                                                         const int *__restrict__ flag, long long n_cars, int Z, int T,
                                                         unsigned long long *__restrict__ obj, double *__restrict__ zone_err,
                                                         double *__restrict__ part, int *__restrict__ part_n)
{
    __shared__ double s_e[kObjBlock / 64];
    __shared__ int s_n[kObjBlock / 64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int b = static_cast<int>(blockIdx.y);
    const int z = static_cast<int>(blockIdx.x) * kObjBlock + tid;
    const bool in = z < Z;
    const bool wave_in = static_cast<int>(blockIdx.x) * kObjBlock + (tid & ~63) < Z;  // wave-uniform: the wave holds a zone
    const size_t zt = static_cast<size_t>(Z) * static_cast<size_t>(T);
    const long long *__restrict__ park = counts + static_cast<size_t>(b) * (2 * zt + 2);
    const long long *__restrict__ drv = park + zt;
    unsigned long long *rec = obj + static_cast<size_t>(b) * static_cast<size_t>(kObjHead + 2 * T);

    long long cmin = 0x7fffffffffffffffll, cmax = -0x7fffffffffffffffll - 1;
    for (int t = 0; t < T; ++t) {
        const size_t i = static_cast<size_t>(t) * Z + z;
        long long p = in ? park[i] : 0ll, d = in ? drv[i] : 0ll;
        if (in) {
            cmin = p < cmin ? p : cmin;
            cmax = p > cmax ? p : cmax;
        }
        for (int o = 32; o > 0; o >>= 1) {
            p += __shfl_down(p, o, 64);
            d += __shfl_down(d, o, 64);
        }
        if (lane == 0 && wave_in) {
            atomicAdd(rec + kObjHead + t, static_cast<unsigned long long>(d));
            atomicAdd(rec + kObjHead + T + t, static_cast<unsigned long long>(p));
        }
    }

    const bool valid = in && measured != nullptr && flag[z] != 0 && cmin != cmax;
    double e = 0.0;
    if (valid) {
        const double n = static_cast<double>(n_cars);
        const double lo = static_cast<double>(cmin) / n, hi = static_cast<double>(cmax) / n;
        const double range = hi - lo;
        double acc = 0.0;
        for (int t = 0; t < T; ++t) {
            const size_t i = static_cast<size_t>(t) * Z + z;
            const double p = static_cast<double>(park[i]) / n;
            const double d = (p - lo) / range - measured[i];
            acc = acc + d * d;
        }
        e = acc / static_cast<double>(T);
    }
    if (in && zone_err) zone_err[static_cast<size_t>(b) * Z + z] = valid ? e : -1.0;

    const double we = obj_wave_sum(e);
    int wn = valid ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) wn += __shfl_down(wn, o, 64);
    if (lane == 0) {
        s_e[wave] = we;
        s_n[wave] = wn;
    }
    __syncthreads();
    if (tid == 0) {
        const size_t k = static_cast<size_t>(b) * gridDim.x + blockIdx.x;
        part[k] = ((s_e[0] + s_e[1]) + s_e[2]) + s_e[3];
        part_n[k] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    }
}

// grid = B, one wave.  Words 0..3 of every record; the hour sums are k_obj_zones' and are not touched.
__global__ __launch_bounds__(64) void k_obj_final(const long long *__restrict__ counts, const double *__restrict__ part,
                                                  const int *__restrict__ part_n, int nb, int Z, int T, unsigned long long *__restrict__ obj)
{
    const int lane = static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.x);
    double s = 0.0;
    int n = 0;
    for (int i = lane; i < nb; i += 64) {
        s = s + part[static_cast<size_t>(b) * nb + i];
        n += part_n[static_cast<size_t>(b) * nb + i];
    }
    s = obj_wave_sum(s);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if (lane == 0) {
        const size_t zt = static_cast<size_t>(Z) * static_cast<size_t>(T);
        const long long *tail = counts + static_cast<size_t>(b) * (2 * zt + 2) + 2 * zt;
        unsigned long long *rec = obj + static_cast<size_t>(b) * static_cast<size_t>(kObjHead + 2 * T);
        const long long status = tail[1];
        rec[0] = static_cast<unsigned long long>(status);
        rec[1] = static_cast<unsigned long long>(tail[0]);
        rec[2] = static_cast<unsigned long long>(n);
        const double err = s / static_cast<double>(n);
        rec[3] = (n == 0 || status != 0) ? 0x7ff8000000000000ull : static_cast<unsigned long long>(__double_as_longlong(err));
    }
}

}  // namespace cpm
