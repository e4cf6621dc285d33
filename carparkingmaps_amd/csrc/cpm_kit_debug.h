// cpm_kit_debug.h -- diagnostic kernels of the travel-time sampler's f64 kit (cpm_debug_travel_draw, cpm_debug_f64_kit, include/cpm.h).
//
// A resample reaches only what its uniforms reach: |u - 1/2| within ~1e-11 of 1/2 (the r > 5 rational of ppnd_tail), u = 0 (its
// val = 9 exit) and the two clamps of truncnormal_draw are never drawn.  These kernels hand given arguments to the SAME inline
// functions the travel kernels call (cpm_rng.h), in this translation unit and under its flags, so that every branch can be compared
// with the CPU restatement bit for bit.  One thread per element; no tables, no datamatrix.
#pragma once
#include "cpm_rng.h"

namespace cpm {

// the statements of a travel kernel for one driver: sigma = std, or a tenth of the mean where the data hold none (src/resampling.jl:65-67),
// the window's mass, u = k * 2^-53 (k: the 53 high bits of the draw, as u53 makes them), the draw, its q16 word
__global__ __launch_bounds__(256) void k_debug_travel_draw(int64_t n, const uint64_t *__restrict__ k53, const double *__restrict__ mean,
                                                           const double *__restrict__ sd, double *__restrict__ draw_out,
                                                           double *__restrict__ mass_out, long long *__restrict__ q16_out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double m = mean[i], s = sd[i];
    const double s1 = (s == 0) ? 0.1 * m : s;
    const double mass = truncnormal_mass(m, s1);
    const double u = static_cast<double>(k53[i] & ((1ull << 53) - 1ull)) * 0x1.0p-53;
    const double x = truncnormal_draw(u, m, s1, mass);
    draw_out[i] = x;
    mass_out[i] = mass;
    q16_out[i] = q16(x);
}

// fn: CPM_KIT_* of include/cpm.h
__global__ __launch_bounds__(256) void k_debug_f64_kit(int fn, int64_t n, const double *__restrict__ x, double *__restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r;
    switch (fn) {
    case 0: r = det_log(v); break;
    case 1: r = det_sqrt(v); break;
    case 2: r = det_erf(v); break;
    case 3: r = ppnd(v); break;
    default: r = exp_neg(v); break;
    }
    out[i] = r;
}

}  // namespace cpm
