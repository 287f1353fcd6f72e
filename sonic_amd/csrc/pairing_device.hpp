// The device pairing as the rest of the library sees it (pairing.hip).
#pragma once
#include "common.hpp"
#include "g2.hpp"

namespace sonic {

// One product check per group: the Miller loops of n pairs of validated points (Montgomery, affine; a pair with either point at
// infinity contributes 1), the product of each group -- group g is the pairs [d_group_end[g-1], d_group_end[g]), all arrays on the
// device -- and its final exponentiation.  d_is_one[g] = 1 when the group's value is one; d_gt (may be null) gets G x 576 bytes, the
// layout of sonic_srs_pairing.  Waits for the stream before it returns: the intermediate values live in buffers of the call.
void pairing_groups_device(hipStream_t st, const G1Affine* dP, const G2Affine* dQ, long n, const int64_t* d_group_end, long G, uint8_t* d_is_one, uint8_t* d_gt);

// the environment's SONIC_PAIRING_GPU, read per call: 0 never the device form, 1 always, -1 (unset or anything else) the rules below
int pairing_gpu_knob();

// The AUTO rules, from profiles/r20_pairing.txt (tools/pairing.py on one MI355X): the smallest measured size from which the device form
// beat the host form by more than the larger of the two spreads, there and at every larger measured size.
//   sonic_pairing_check, where = SONIC_PAIRING_AUTO: groups in the call (section (a): groups of 4 pairs)
//   verify_batch(each=True) after a failed fold:    proofs in the batch (section (b))
constexpr int64_t PAIRING_GPU_MIN_GROUPS = 256;      // (a): 77.0 ms on the host against 41.9 ms at G = 256; NOT held at G = 64 (20.5 against 41.7)
constexpr int64_t EACH_GPU_MIN_PROOFS = 64;          // (b): 183.7 ms against 73.2 ms at K = 64; NOT held at K = 16 (52.1 against 74.9)

}  // namespace sonic
