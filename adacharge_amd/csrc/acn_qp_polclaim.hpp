// The claim step of a polish launch that runs ALONGSIDE the solver launch filling its list.
//
// Producers (the solver's waves) reserve a slot with a fetch-add on the list length and then publish the problem index
// into it with a release store; the list is preset to -1.  When a producer is through with all its problems it adds
// their number to `retired` (release).  Consumers (one thread per polish workgroup) run pol_claim:
//   - an entry is claimed only once it EXISTS: read list[head] (acquire); >= 0: compare-and-swap the shared queue
//     counter head -> head + 1; the winner owns position head.  Nobody ever holds a ticket for an unpublished entry, so
//     a consumer that gives up loses nothing, and the counter always equals the number of entries claimed: the serial
//     launch behind the solver goes on from it with its fetch-add;
//   - no entry pending: once retired == expected (acquire: every publication is visible then) one more look at
//     list[head] tells a drained list (kPolClaimDrained) from a late entry;
//   - otherwise pause and poll again.  A poll is one look at the head of the list, whatever it finds, and one call makes
//     at most max_polls of them (kPolClaimGaveUp): no wait here is unbounded, and a bound of 0 leaves without a look.
// Host-compilable: tests/host/polish_claim_threads.cpp plays both sides with threads under a sanitizer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ACNQP_CLAIM_FN __host__ __device__ inline
#else
#define ACNQP_CLAIM_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define ACNQP_CLAIM_LOAD_ACQ(p) __hip_atomic_load((p), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)
#define ACNQP_CLAIM_CAS(p, expect, want) \
  __hip_atomic_compare_exchange_strong((p), (expect), (want), __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)
#else
#define ACNQP_CLAIM_LOAD_ACQ(p) __atomic_load_n((p), __ATOMIC_ACQUIRE)
#define ACNQP_CLAIM_CAS(p, expect, want) __atomic_compare_exchange_n((p), (expect), (want), false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)
#endif

namespace acnqp {

constexpr int kPolClaimDrained = -1;   // the producers are through and the list holds nothing unclaimed
constexpr int kPolClaimGaveUp = -2;    // the poll bound ran out (the serial launch polishes what is left)

// `capacity`: entries the list holds (the batch).  `pause()`: what a consumer does between two polls.
template <class Pause>
ACNQP_CLAIM_FN int pol_claim(const int32_t* list, int32_t* queue, const int32_t* retired, int32_t expected, int32_t capacity,
                             long long max_polls, Pause pause) {
  long long polls = 0;
  for (;;) {
    if (polls >= max_polls) return kPolClaimGaveUp;   // (ahead of the look: a bound of 0 takes nothing at all)
    ++polls;
    int32_t head = ACNQP_CLAIM_LOAD_ACQ(queue);
    if (head >= capacity) return kPolClaimDrained;
    if (ACNQP_CLAIM_LOAD_ACQ(list + head) >= 0) {
      if (ACNQP_CLAIM_CAS(queue, &head, head + 1)) return head;
      continue;   // another consumer took it: look at the new head
    }
    if (ACNQP_CLAIM_LOAD_ACQ(retired) >= expected) {
      if (ACNQP_CLAIM_LOAD_ACQ(list + head) < 0) return kPolClaimDrained;
      continue;
    }
    pause();
  }
}

}  // namespace acnqp
