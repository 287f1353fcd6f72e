// The prover's streams as one pool per device ("Two streamed small proofs and the chip").  Host only: no HIP type
// appears here, so the mapping and the parsing are tested by a stand-alone program (tests/host/stream_pool_host.cpp).
//
// The runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the environment says otherwise) round-robin in creation
// order, and streams that share a queue run behind each other.  A handle with eight streams of its own, two such handles and the
// device's stream are 17 streams: which of one proof's accumulations the other proof's small head kernels queue behind was an accident
// of the order in which the handles were made.  The pool has no more streams than there are queues, every handle borrows them, and the
// ROLE of a piece of work decides its stream -- the same for every handle, so the head of the next proof never sits behind the body of
// the one before it.
#pragma once
#include <stdlib.h>

namespace sonic {

constexpr int POOL_MIN = 2, POOL_MAX = 32;      // streams in a pool (SONIC_STREAM_POOL=k may force any of these)
constexpr int POOL_CAP = 8;                     // what the library takes of the queues by itself: a proof has no more roles that overlap
constexpr int POOL_DEFAULT_QUEUES = 4;          // the runtime's own default when GPU_MAX_HW_QUEUES is unset
// Does a handle borrow pool streams when SONIC_STREAM_POOL is unset?  Yes: ms per streamed proof at n = 2^18, private streams / pool,
// 33.5 / 31.8 on the runtime's 4 queues and 31.8 / 31.1 on 8 (profiles/r13_stream_pool.txt).
constexpr bool POOL_DEFAULT_ON = true;

// What a stream is used for inside one proof, in the order in which a proof queues them:
//   HEAD     transcript upload, the polynomials, the small side MSMs
//   NTT      the t(X,y) product
//   GROUP    k: the lane of the k-th group of MSMs (R W_a W_b | S_j W_j W'_j | C Q_j Q_v)
//   T_GROUP  the lane of the t group (T, W_t): the largest, ready last and queued last
//   CHAIN    c: the one chain of a fused (small) proof
//   TAIL     the join over the lanes and the copy-out of slots, evaluations and flags
enum class PoolRole { HEAD, NTT, GROUP, T_GROUP, CHAIN, TAIL };

// The stream, below P, of a role in a pool of P >= 2 streams.  Three rules hold for every P (checked by the host test):
//   1. TAIL never shares a stream with HEAD or NTT: the next proof's head would wait for the whole proof before it.
//   2. TAIL shares a stream only with the body of a proof that is queued last: T_GROUP, and below P = 6 the chains of fused proofs -- no
//      GROUP, except at P = 2, where rules 1 and 3 leave one stream for everything that is neither HEAD nor NTT.
//   3. HEAD shares with no GROUP, T_GROUP or CHAIN; only at P = 2 does it share with NTT.
// Within them the groups go round-robin over the streams that are left.  NTT has a stream to itself from P = 5; at P = 3 and 4 (the
// runtime's default number of queues) it shares the first group stream, and GROUP(0), which is queued right behind it and needs nothing
// but r(X,1), starts on the next one.  A fused proof's lanes only prepare openings -- its t lane too, which is therefore a GROUP for a
// small-proof handle (prove.hip) -- and its chain is its whole body: on a stream that a chain uses, the next proof's preparation would
// wait for that chain, so no group shares one.  From P = 6 the chains have a stream to themselves; below, they run on TAIL's.
inline int pool_stream_of(PoolRole role, int k, int P) {
  if (P < POOL_MIN) P = POOL_MIN;
  if (k < 0) k = 0;
  if (P == 2) return role == PoolRole::HEAD || role == PoolRole::NTT ? 0 : 1;
  const bool ntt_alone = P >= 5, chain_alone = P >= 6;
  const int first = ntt_alone ? 2 : 1, cnt = P - 1 - first - (chain_alone ? 1 : 0);      // the group streams: first .. first + cnt - 1
  switch (role) {
    case PoolRole::HEAD: return 0;
    case PoolRole::NTT: return 1;
    case PoolRole::TAIL:
    case PoolRole::T_GROUP: return P - 1;
    case PoolRole::CHAIN: return chain_alone ? P - 2 : P - 1;
    case PoolRole::GROUP: return first + (k + (ntt_alone ? 0 : 1)) % cnt;
  }
  return 0;
}

// GPU_MAX_HW_QUEUES as the runtime reads it: unset or unparsable is its default of 4; clamped to what a pool can be.  Read, never set:
// the variable only counts when it is in the environment before the process's first HIP call, which a library cannot arrange.
inline int pool_queues_of_env(const char* v) {
  if (!v || !*v) return POOL_DEFAULT_QUEUES;
  char* end = nullptr;
  const long q = strtol(v, &end, 10);
  if (end == v || *end) return POOL_DEFAULT_QUEUES;
  return q < POOL_MIN ? POOL_MIN : q > POOL_MAX ? POOL_MAX : (int)q;
}

// The size of a device's pool, decided once when it is made; 0: no pool, every handle makes private streams.
//   SONIC_STREAM_POOL unset   the default (POOL_DEFAULT_ON): min(queues, POOL_CAP) streams, or none
//   SONIC_STREAM_POOL=0       private streams (A/B runs, and the fallback)
//   SONIC_STREAM_POOL=k       k streams, clamped to POOL_MIN .. POOL_MAX (tests); anything unparsable counts as unset
inline int pool_size_of_env(const char* queues, const char* knob, bool default_on = POOL_DEFAULT_ON) {
  const int q = pool_queues_of_env(queues);
  const int by_queues = q < POOL_CAP ? q : POOL_CAP;
  if (knob && *knob) {
    char* end = nullptr;
    const long k = strtol(knob, &end, 10);
    if (end != knob && !*end) return k <= 0 ? 0 : k < POOL_MIN ? POOL_MIN : k > POOL_MAX ? POOL_MAX : (int)k;
  }
  return default_on ? by_queues : 0;
}

}  // namespace sonic
