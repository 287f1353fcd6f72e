// Internal interface of the G2 multi-scalar multiplication (msm_g2.hip): the bucket method on the twist, behind the sort phase it
// shares with the G1 MSM (msm.hpp, msm_sort_enqueue).  The host-only parts -- window rule, shifts, Horner fold, chunk cut: msm_g2_host.hpp.
#pragma once
#include "internal.hpp"
#include "g2.hpp"
#include "msm_g2_host.hpp"

namespace sonic {

// sum_i scalars[i] * pts[i] over n > 0 points as the 192 canonical bytes sonic_srs_get_g2_points writes (zeros: the point at infinity).
// d_scalars: resident, standard form, below 2^(bits - 1) (msm_g2_host.hpp).  fold: scalars above (r - 1) / 2 run as r - s on the negated
// point -- only for points of the order-r subgroup (SRS elements); without it the sum is the literal multiple.  Slabs of G2_MSM_SLAB
// terms, one chain each on the workspace; waits for the stream.
void g2_msm_blocking(hipStream_t st, MsmWorkspace& ws, const G2Affine* pts, const Fr* d_scalars, long n, int bits, bool fold, uint8_t out192[192]);

// caller-supplied points (sonic_msm_g2): canonical coordinates on the twist, or 192 zero bytes for the point at infinity; no subgroup test.
// err bits: 1 non-canonical, 2 off the curve
void g2_msm_points_from_bytes_enqueue(hipStream_t st, const uint8_t* d_in, G2Affine* out, long n, int* d_err);

// k_g2_sum over several ranges (srs_g2.hip)
void g2_sum_ranges_enqueue(hipStream_t st, const G2Jac* in, long n, int ranges, long range_stride, G2Jac* tmp, G2Jac* tot);
constexpr int G2_SUM_RANGE_BLOCKS = 64;      // points per range `tmp` must hold

}  // namespace sonic
