// Stand-alone host check of the claim step of the polish launch that runs alongside the solver launch
// (adacharge_amd/csrc/acn_qp_polclaim.hpp): threads play the solver's waves (producers) and the polish workgroups
// (consumers).  Built with -fsanitize=thread by tests/test_polish_claim_host.py; no GPU, no Python inside.
//
//   polish_claim_threads [producers] [consumers] [problems] [rounds]
//
// Every round: each producer takes problems from a shared queue, writes a payload for each with PLAIN stores, hands about
// a third of them over (reserve a slot, publish with a release store) and, when the queue is empty, adds the number of
// problems it took to `retired`.  Consumers claim entries with pol_claim, read the payload with PLAIN loads (the sanitizer
// checks that the publication orders them) and count their visit.  Odd-numbered consumers give up after a handful of
// polls.  Afterwards the "serial launch" goes on from the queue counter with a fetch-add, as the kernel does.  Checked:
// every handed-over problem is visited exactly once, the counter ends at the list length, nothing else was visited.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "acn_qp_polclaim.hpp"

namespace {

struct Shared {
  int problems = 0;
  std::vector<int32_t> list;      // preset to -1
  int32_t queue = 0;              // entries claimed
  int32_t count = 0;              // entries reserved
  int32_t retired = 0;            // problems finished
  int32_t next = 0;               // the producers' work queue
  std::vector<long long> payload; // written by the producer of the problem, read by its consumer
  std::vector<int> visits;        // written by the consumer
  std::vector<char> handed;       // written by the producer, read after the join
};

long long payload_of(int b, int round) { return 1000003ll * b + 7919ll * round + 1; }

void producer(Shared* s, int round, unsigned seed) {
  int took = 0;
  for (;;) {
    const int b = __atomic_fetch_add(&s->next, 1, __ATOMIC_RELAXED);
    if (b >= s->problems) break;
    ++took;
    seed = seed * 1664525u + 1013904223u;
    for (volatile int spin = (seed >> 20) & 255; spin > 0; --spin) {}   // problems take different times
    s->payload[b] = payload_of(b, round);
    const bool hand = ((seed >> 8) % 3) == 0;
    s->handed[b] = hand ? 1 : 0;
    if (hand) {
      const int slot = __atomic_fetch_add(&s->count, 1, __ATOMIC_RELAXED);
      __atomic_store_n(&s->list[slot], b, __ATOMIC_RELEASE);
    }
  }
  if (took > 0) __atomic_fetch_add(&s->retired, took, __ATOMIC_RELEASE);
}

void consumer(Shared* s, int round, long long max_polls, int* bad) {
  for (;;) {
    const int pos = acnqp::pol_claim(s->list.data(), &s->queue, &s->retired, s->problems, s->problems, max_polls, [] { std::this_thread::yield(); });
    if (pos < 0) return;
    const int b = __atomic_load_n(&s->list[pos], __ATOMIC_ACQUIRE);
    if (b < 0 || b >= s->problems || s->payload[b] != payload_of(b, round)) { ++*bad; continue; }
    s->visits[b] += 1;
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int producers = argc > 1 ? std::atoi(argv[1]) : 6;
  const int consumers = argc > 2 ? std::atoi(argv[2]) : 4;
  const int problems = argc > 3 ? std::atoi(argv[3]) : 3000;
  const int rounds = argc > 4 ? std::atoi(argv[4]) : 20;
  int failures = 0;
  long long alongside = 0, serial = 0;
  for (int round = 0; round < rounds; ++round) {
    Shared s;
    s.problems = problems;
    s.list.assign(problems, -1);
    s.payload.assign(problems, 0);
    s.visits.assign(problems, 0);
    s.handed.assign(problems, 0);
    std::vector<int> bad(consumers, 0);
    std::vector<std::thread> th;
    // (consumers first in every other round: a polish launch may well start ahead of the solver)
    auto start_consumers = [&] {
      for (int c = 0; c < consumers; ++c) th.emplace_back(consumer, &s, round, (c & 1) ? 3ll : (1ll << 40), &bad[c]);
    };
    if (round & 1) start_consumers();
    for (int p = 0; p < producers; ++p) th.emplace_back(producer, &s, round, 977u * (unsigned)(round * producers + p) + 1u);
    if (!(round & 1)) start_consumers();
    for (auto& t : th) t.join();
    alongside += s.queue;
    // the serial launch: from the same counter up to the list length
    for (;;) {
      const int pos = __atomic_fetch_add(&s.queue, 1, __ATOMIC_RELAXED);
      if (pos >= s.count) break;
      const int b = s.list[pos];
      if (b < 0 || b >= problems) { ++failures; continue; }
      s.visits[b] += 1;
      ++serial;
    }
    for (int c = 0; c < consumers; ++c) failures += bad[c];
    if (s.retired != problems) ++failures;
    int handed = 0;
    for (int b = 0; b < problems; ++b) {
      handed += s.handed[b];
      if (s.visits[b] != (s.handed[b] ? 1 : 0)) ++failures;
    }
    if (handed != s.count) ++failures;
    // (a consumer with the long bound only ever returns on a drained list: with one present nothing is left for the serial part)
    for (int pos = s.count; pos < problems; ++pos) if (s.list[pos] != -1) ++failures;
  }
  std::printf("{\"rounds\": %d, \"alongside\": %lld, \"serial\": %lld, \"failures\": %d}\n", rounds, alongside, serial, failures);
  return failures == 0 ? 0 : 1;
}
