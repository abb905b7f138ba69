// Drives the host half of the flagged-word protocol (mimosa_amd/csrc/flagged_word.hpp) on the CPU for
// tests/test_flagged_word_cpu.py.  A word is written the way the device writes it — four dwords {lo, seq, hi, seq} — and read
// back with ll_read_bits / ll_read; the bounded spin is timed with a predicate that never holds.  stdout: JSON.
#include <chrono>
#include <cstdio>
#include <cstring>

#include "flagged_word.hpp"

static void put(uint64_t * q, unsigned long long bits, unsigned int seq_lo, unsigned int seq_hi)
{
  const uint32_t w[4] = {static_cast<uint32_t>(bits), seq_lo, static_cast<uint32_t>(bits >> 32), seq_hi};
  std::memcpy(q, w, sizeof(w));
}

int main()
{
  alignas(16) uint64_t q[2];
  unsigned long long got = 0x1111111111111111ull;
  double v = 1.5;

  // the two halves carry different sequence numbers (a store of call 7 has landed on one half of call 6's word)
  put(q, 0x0123456789abcdefull, 7u, 6u);
  const bool torn_a = mh::ll_read_bits(q, 7u, got) || mh::ll_read_bits(q, 6u, got) || mh::ll_read(q, 7u, v);
  put(q, 0x0123456789abcdefull, 6u, 7u);
  const bool torn_b = mh::ll_read_bits(q, 7u, got) || mh::ll_read_bits(q, 6u, got) || mh::ll_read(q, 6u, v);
  // a complete word of an earlier call
  put(q, 0x0123456789abcdefull, 6u, 6u);
  const bool stale = mh::ll_read_bits(q, 7u, got) || mh::ll_read(q, 7u, v);
  const bool untouched = got == 0x1111111111111111ull && v == 1.5;  // a refused read writes nothing

  // a matching word gives back the 64 bits that were stored: NaN payloads, -0.0, denormals, all ones
  const unsigned long long pats[] = {0x7ff8000000000001ull, 0xfff4dead0000beefull, 0x7ff0000000000001ull, 0x8000000000000000ull, 0x0000000000000001ull,
                                     0xffffffffffffffffull, 0x0000000000000000ull, 0x3ff0000000000000ull, 0x00000007ffffffffull, 0xfffffff800000000ull};
  std::printf("{\"torn_a\": %d, \"torn_b\": %d, \"stale\": %d, \"untouched\": %d, \"exact\": [", torn_a, torn_b, stale, untouched);
  unsigned int seq = 0xfffffffeu;  // across the wrap of the counter, 0 left out as next_call_seq leaves it out
  for (size_t i = 0; i < sizeof(pats) / sizeof(pats[0]); ++i) {
    put(q, pats[i], seq, seq);
    unsigned long long bits = 0;
    double d = 0.0;
    unsigned long long dbits = 0;
    const bool ok = mh::ll_read_bits(q, seq, bits) && mh::ll_read(q, seq, d);
    std::memcpy(&dbits, &d, sizeof(d));
    std::printf("%s%d", i ? ", " : "", ok && bits == pats[i] && dbits == pats[i]);
    if (++seq == 0u) ++seq;
  }

  // the bounded spin: no budget = one look, no wait; a budget = false once it has passed
  auto ms_of = [](long budget_ns, long & looks) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool r = mh::spin_until([&] { ++looks; return false; }, budget_ns);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return r ? -1.0 : ms;
  };
  long looks0 = 0, looksn = 0, looks1 = 0, looks_true = 0;
  const double ms0 = ms_of(0L, looks0), msn = ms_of(-5L, looksn), ms1 = ms_of(1000000L, looks1);
  const bool holds = mh::spin_until([&] { return ++looks_true == 3; }, 1000000000L) && mh::spin_until([] { return true; }, 0L);
  std::printf("], \"looks_zero\": %ld, \"looks_negative\": %ld, \"ms_zero\": %.6f, \"ms_negative\": %.6f, \"ms_1ms\": %.6f, \"looks_1ms\": %ld, \"holds\": %d, \"looks_holds\": %ld}\n",
              looks0, looksn, ms0, msn, ms1, looks1, holds, looks_true);
  return 0;
}
