// cpm_expected_var.h -- exact variances of a resample's counts from the day's transition matrix (include/cpm_expected_var.h):
// k_var_eye, k_var_gemm, k_var_reduce, k_var_final.
//
// The product P <- P * M_t is an "NT" GEMM on v_mfma_f64_16x16x4_f64: P is stored [start s][origin o] and the hour's block of p
// [dest d][origin o], so both operands are contiguous along the summed index o.  A workgroup of 256 threads (four waves, 2 x 2)
// computes a 128 x 128 tile of the result; a wave holds a 64 x 64 quarter as 4 x 4 MFMA tiles (16 accumulators of 4 f64).  The
// summed index goes through LDS in slices of 16: both slices are stored [k][row] with a row pitch of 144 words, so that the 16
// lanes of one k read 16 consecutive words and the lane groups of k and k + 1 sit 128 bytes apart modulo the 256 bytes of the banks
// (no conflict within a half wave).  The next slice's global loads are issued into registers before the MFMAs of the current one and
// stored to LDS behind them (one LDS buffer, two barriers per slice; no arithmetic touches a loaded word in front of the MFMAs, or
// the compiler's wait for it would stand there too): a slice is 64 MFMAs of 64 cycles per wave, against 16 scalar
// loads per lane, so the matrix pipe is what the kernel waits for and a second LDS buffer buys nothing measurable.  128 x 128 makes
// 16 flop per byte loaded from the L2.
//
// M_t's slice is formed while it is staged: a thread stages ONE origin o of the slice (and eight destinations), so it reads q[o],
// r[o], l[o] and the row total once per slice, scales its eight p words and adds the residual and the staying mass where its
// destination is l[o] or o.  The whole operator is one GEMM: no gather behind it.
//
// Edges: the loads are scalar (8 bytes: a row of p starts off a 16-byte line when Z is odd) and their indices clamped to Z - 1; what
// lies past Z is staged as +0, in the summed index too (a K remainder of 1, 2 or 3 adds fma(0, 0, acc): no bit changes), and the stores of the
// epilogue are bounds-checked.
//
// The four weighted column sums of an hour take a pass of their own over P (Z * Z words against the product's 2 * Z^3 flop): a thread
// owns a destination and adds kVarRedRows start rows in ascending order; k_var_final adds the chunks in ascending order.  No
// floating-point atomics: the order of every sum is a function of Z alone.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected.h"

namespace cpm {

constexpr int kVarBlock = 256;
constexpr int kVarTile = 128;    // rows and columns of a workgroup's tile (a wave: 64 x 64)
constexpr int kVarK = 16;        // the summed index per LDS slice (four MFMA steps)
constexpr int kVarPitch = 144;   // words between two k of a staged slice (see above)
constexpr int kVarStage = kVarTile * kVarK / kVarBlock;  // words a thread stages per operand and slice
constexpr int kVarRedRows = 64;  // start rows of one partial sum
static_assert(kVarStage == 8 && kVarBlock / kVarK == 16, "k_var_gemm stages rows tid / 16 + 16 i");

typedef double var_f64x4 __attribute__((ext_vector_type(4)));

// P_0 = I.  grid = ceil(Z * Z / 256)
__global__ __launch_bounds__(kVarBlock) void k_var_eye(double *__restrict__ P, int Z)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * kVarBlock + threadIdx.x;
    const size_t n = static_cast<size_t>(Z) * Z;
    if (i < n) P[i] = (i / Z == i % Z) ? 1.0 : 0.0;
}

// Pout = P * M_t.  grid = (ceil(Z / 128) destinations, ceil(Z / 128) start rows).  p_t / last_t / r_t / ell_t / pd_t: the hour's slices.
// Two workgroups per CU (240 registers a lane, no spill): one's MFMAs cover the other's barriers and LDS stores.
__global__ __launch_bounds__(kVarBlock, 2) void k_var_gemm(const double *__restrict__ P, const double *__restrict__ p_t, const double *__restrict__ last_t,
                                                        const double *__restrict__ r_t, const int *__restrict__ ell_t,
                                                        const double *__restrict__ pd_t, double *__restrict__ Pout, int Z)
{
    __shared__ double s_a[kVarK * kVarPitch];
    __shared__ double s_b[kVarK * kVarPitch];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int m0 = static_cast<int>(blockIdx.y) * kVarTile, n0 = static_cast<int>(blockIdx.x) * kVarTile;
    const int kk = tid & (kVarK - 1), rr = tid >> 4;  // this thread stages origin k0 + kk of rows rr + 16 i

    var_f64x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = var_f64x4{0.0, 0.0, 0.0, 0.0};

    // what a thread holds of the slice in flight: the raw words of P and p, and its origin's p_drive, row total, r and l.  M_t's words are
    // formed from them at the LDS store, BEHIND the MFMAs of the slice before: nothing in front of those MFMAs waits for a load.
    double ra[kVarStage], rb[kVarStage];
    double fpd = 0.0, flast = 0.0, fr = 0.0;
    int fo = 0, fell = -1;
    auto fetch = [&](int k0) {
        fo = k0 + kk;
        const int oc = fo < Z ? fo : Z - 1;  // (clamped: the loads stay inside, the words are dropped at the store)
        fpd = pd_t[oc];
        flast = last_t[oc];
        fell = ell_t[oc];
        fr = r_t[oc];
#pragma unroll
        for (int i = 0; i < kVarStage; ++i) {
            const int sr = m0 + rr + 16 * i, dr = n0 + rr + 16 * i;
            ra[i] = P[static_cast<size_t>(sr < Z ? sr : Z - 1) * Z + oc];
            rb[i] = p_t[static_cast<size_t>(dr < Z ? dr : Z - 1) * Z + oc];
        }
    };
    auto stage = [&]() {
        const bool in_k = fo < Z, zero = flast == 0.0;
        const double q = exp_q(fpd), qr = q * fr, stay = 1.0 - q;
#pragma unroll
        for (int i = 0; i < kVarStage; ++i) {
            const int sr = m0 + rr + 16 * i, d = n0 + rr + 16 * i;
            double v = rb[i] * q;
            v = d == fell ? v + qr : v;
            v = d == fo ? v + stay : v;
            // a zero row: the driver stays where it is, so all of q[o] and of 1 - q[o] is at d = o
            v = zero ? (d == fo ? 1.0 : 0.0) : v;
            s_a[kk * kVarPitch + rr + 16 * i] = (in_k && sr < Z) ? ra[i] : 0.0;
            s_b[kk * kVarPitch + rr + 16 * i] = (in_k && d < Z) ? v : 0.0;
        }
    };

    fetch(0);
    for (int k0 = 0; k0 < Z; k0 += kVarK) {
        __syncthreads();  // (the MFMAs of the slice before have read their words)
        stage();
        __syncthreads();
        if (k0 + kVarK < Z) fetch(k0 + kVarK);
#pragma unroll
        for (int ks = 0; ks < kVarK / 4; ++ks) {
            // A: lane l holds A[row l & 15][k l >> 4]; B: B[k l >> 4][column l & 15]
            const int at = (ks * 4 + (lane >> 4)) * kVarPitch + (lane & 15);
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = s_a[at + wm + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = s_b[at + wn + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 * register (NOT the f32 map)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn + 16 * j + (lane & 15);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = m0 + wm + 16 * i + (lane >> 4) + 4 * g;
                if (row < Z && col < Z) Pout[static_cast<size_t>(row) * Z + col] = acc[i][j][g];
            }
        }
}

// The partial sums of hour t over start rows [64 y, 64 y + 64): part[y][4][Z], mean_parking, mean_driving, var_parking, var_driving.
// grid = (ceil(Z / 256), ceil(Z / 64)).  w: nullptr = 1 per zone.  Every step is one IEEE operation; 1 - P is clamped at 0 (its exact
// value is not negative).
__global__ __launch_bounds__(kVarBlock) void k_var_reduce(const double *__restrict__ P, const double *__restrict__ w, const double *__restrict__ pd_t, int Z,
                                                          double *__restrict__ part)
{
    const int z = static_cast<int>(blockIdx.x) * kVarBlock + static_cast<int>(threadIdx.x);
    if (z >= Z) return;
    const double q = exp_q(pd_t[z]);
    const int s0 = static_cast<int>(blockIdx.y) * kVarRedRows, s1 = s0 + kVarRedRows < Z ? s0 + kVarRedRows : Z;
    double mp = 0.0, md = 0.0, vp = 0.0, vd = 0.0;
    for (int s = s0; s < s1; ++s) {
        const double ws = w ? w[s] : 1.0;
        const double pv = P[static_cast<size_t>(s) * Z + z];
        const double a = pv * q;
        double np = 1.0 - pv, na = 1.0 - a;
        np = np > 0.0 ? np : 0.0;
        na = na > 0.0 ? na : 0.0;
        mp = mp + ws * pv;
        md = md + ws * a;
        vp = vp + ws * (pv * np);
        vd = vd + ws * (a * na);
    }
    double *const o = part + static_cast<size_t>(blockIdx.y) * 4 * Z + z;
    o[0] = mp;
    o[static_cast<size_t>(Z)] = md;
    o[2 * static_cast<size_t>(Z)] = vp;
    o[3 * static_cast<size_t>(Z)] = vd;
}

// out[k][t][z] = the chunks' partial sums in ascending order.  grid = (ceil(Z / 256), 4)
__global__ __launch_bounds__(kVarBlock) void k_var_final(const double *__restrict__ part, int chunks, int Z, int T, int t, double *__restrict__ out)
{
    const int z = static_cast<int>(blockIdx.x) * kVarBlock + static_cast<int>(threadIdx.x), k = static_cast<int>(blockIdx.y);
    if (z >= Z) return;
    double v = 0.0;
    for (int y = 0; y < chunks; ++y) v = v + part[(static_cast<size_t>(y) * 4 + k) * Z + z];
    out[(static_cast<size_t>(k) * T + t) * Z + z] = v;
}

}  // namespace cpm
