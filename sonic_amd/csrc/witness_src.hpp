// Witness sources (include/sonic_hip.h, "Witness sources"): where an assignment comes from -- host or device memory, 32-byte canonical Fr
// or signed 64-bit integers, aO given or derived -- as one description, written once for the host and the device.  The conversion of an
// int64 to a field element and the checks of a sonic_witness_src_t that need no device are the text below; the kernel of witness_src.hip
// and the host program of tests/host/witness_src_host.cpp compile the same functions.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "../../include/sonic_hip.h"
#include "field.hpp"

namespace sonic {

// v >= 0 is v, v < 0 is r - |v|, in standard form (below r: |v| <= 2^63 < r).  |v| is formed in unsigned arithmetic, where the negation
// of INT64_MIN is 2^63 and nothing overflows.
HD Fr wit_i64_to_fr(int64_t v) {
  const bool neg = v < 0;
  const uint64_t mag = neg ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
  Fr m = Fr::zero();
  m.l[0] = (uint32_t)mag;
  m.l[1] = (uint32_t)(mag >> 32);
  if (!neg) return m;
  Fr out;
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < FR_LIMBS; i++) {
    const uint64_t d = (uint64_t)FrParams::p(i) - m.l[i] - br;
    out.l[i] = (uint32_t)d;
    br = (d >> 32) & 1;
  }
  return out;
}

HD int wit_elem_bytes(int kind) { return kind == SONIC_WIT_I64 ? 8 : 32; }

// A checked source, on the pattern of CircuitView (csr.hpp): the caller's pointers as bytes, the stride resolved (never 0), aO null when
// it is derived.  Block b of a vector starts at v + b * stride.
struct WitnessView {
  const uint8_t *aL = nullptr, *aR = nullptr, *aO = nullptr;
  int kind = SONIC_WIT_FR32;
  bool on_device = false;
  int64_t stride = 0;            // bytes from assignment b to b + 1
  void* hip_stream = nullptr;    // device sources: the stream whose work produces the data
  int elem() const { return wit_elem_bytes(kind); }
  WitnessView block(int64_t b) const {
    WitnessView w = *this;
    w.aL = aL + b * stride; w.aR = aR + b * stride; w.aO = aO ? aO + b * stride : nullptr;
    return w;
  }
};

// The checks of a description of B assignments of n elements that need no device, before any launch.  SONIC_OK and *out, or
// SONIC_ERR_INVALID_ARG and the reason in msg.
inline int wit_view_checked(const sonic_witness_src_t* s, int64_t n, int64_t B, WitnessView* out, char* msg, size_t cap) {
  if (!s) { snprintf(msg, cap, "the witness source is NULL"); return SONIC_ERR_INVALID_ARG; }
  if (!s->aL || !s->aR) { snprintf(msg, cap, "aL and aR must be given (only aO may be NULL: it is then derived as aL * aR)"); return SONIC_ERR_INVALID_ARG; }
  if (s->kind != SONIC_WIT_FR32 && s->kind != SONIC_WIT_I64) { snprintf(msg, cap, "unknown kind %d (SONIC_WIT_FR32 = 0, SONIC_WIT_I64 = 1)", (int)s->kind); return SONIC_ERR_INVALID_ARG; }
  if (s->on_device != 0 && s->on_device != 1) { snprintf(msg, cap, "on_device = %d is neither 0 (host) nor 1 (device)", (int)s->on_device); return SONIC_ERR_INVALID_ARG; }
  if (n < 1 || B < 1) { snprintf(msg, cap, "need n >= 1 and at least one assignment"); return SONIC_ERR_INVALID_ARG; }
  const int64_t elem = wit_elem_bytes(s->kind), packed = n * elem;
  if (s->stride != 0 && s->stride < packed) { snprintf(msg, cap, "stride %lld is below n * element size = %lld (0 = packed)", (long long)s->stride, (long long)packed); return SONIC_ERR_INVALID_ARG; }
  if (s->on_device) {
    // a device source is read where it lies, with vector loads: 16-byte loads of 32-byte elements, 8-byte loads of integers
    const int64_t align = elem;
    const void* v[3] = {s->aL, s->aR, s->aO};
    const char* name[3] = {"aL", "aR", "aO"};
    for (int k = 0; k < 3; k++)
      if (v[k] && (uintptr_t)v[k] % (uintptr_t)align) { snprintf(msg, cap, "device pointer %s is not %lld-byte aligned", name[k], (long long)align); return SONIC_ERR_INVALID_ARG; }
    if (s->stride % align) { snprintf(msg, cap, "stride %lld of a device source is not a multiple of %lld", (long long)s->stride, (long long)align); return SONIC_ERR_INVALID_ARG; }
  } else if (s->hip_stream) { snprintf(msg, cap, "hip_stream is for device sources (a host source is complete when the call is made)"); return SONIC_ERR_INVALID_ARG; }
  out->aL = static_cast<const uint8_t*>(s->aL); out->aR = static_cast<const uint8_t*>(s->aR); out->aO = static_cast<const uint8_t*>(s->aO);
  out->kind = s->kind; out->on_device = s->on_device != 0; out->stride = s->stride ? s->stride : packed; out->hip_stream = s->hip_stream;
  return SONIC_OK;
}

}  // namespace sonic
