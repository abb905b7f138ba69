// The flagged-word protocol, both halves (layout of a call's slot: icp_device.hpp).  A double travels from a kernel to the
// host as ONE 16-byte store {lo, seq, hi, seq} into mapped pinned memory: each 8-byte half carries the call's sequence
// number, so the host knows a value has arrived by looking at the value itself.  The host half names no HIP type — a flagged
// word is two 64-bit words to it — and is compiled by plain g++ as well (tests/cpp/flagged_word.cpp).
#pragma once

#include <cstdint>
#include <cstring>
#include <ctime>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace mh
{
#ifdef __HIPCC__
// device: 64 bits (a double, or packed counts) as one flagged word.  No arithmetic: the same store whatever the file's
// floating-point contraction setting.
__device__ __forceinline__ void ll_store_bits(uint4 * p, unsigned long long b, unsigned int seq)
{
  *p = make_uint4(static_cast<unsigned int>(b), seq, static_cast<unsigned int>(b >> 32), seq);
}
__device__ __forceinline__ void ll_store(uint4 * p, double v, unsigned int seq)
{
  ll_store_bits(p, static_cast<unsigned long long>(__double_as_longlong(v)), seq);
}
#endif

// host: q = the two self-validating 8-byte halves {lo | seq << 32, hi | seq << 32} of one flagged word
inline bool ll_read_bits(const uint64_t * q, unsigned int seq, unsigned long long & bits)
{
  const unsigned long long a = __atomic_load_n(q, __ATOMIC_ACQUIRE), b = __atomic_load_n(q + 1, __ATOMIC_ACQUIRE);
  if (static_cast<unsigned int>(a >> 32) != seq || static_cast<unsigned int>(b >> 32) != seq) return false;
  bits = (a & 0xffffffffull) | (b << 32);
  return true;
}
inline bool ll_read(const uint64_t * q, unsigned int seq, double & v)
{
  unsigned long long bits;
  if (!ll_read_bits(q, seq, bits)) return false;
  std::memcpy(&v, &bits, sizeof(v));
  return true;
}

// host: the bounded wait for values that arrive by themselves.  until(pred) spins (pause; the clock every 1024 spins) until
// pred() holds: false once budget_ns has passed since construction, or at once when the budget is <= 0.  One object may
// serve a run of waits, which then share the budget.
class SpinBudget
{
public:
  explicit SpinBudget(long budget_ns) : budget_ns_(budget_ns)
  {
    if (budget_ns_ > 0) clock_gettime(CLOCK_MONOTONIC, &t0_);
  }
  template <typename P>
  bool until(P && pred)
  {
    while (!pred()) {
      if (budget_ns_ <= 0) return false;
      __builtin_ia32_pause();
      if ((++spins_ & 1023u) == 0u) {
        timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if ((t1.tv_sec - t0_.tv_sec) * 1000000000L + (t1.tv_nsec - t0_.tv_nsec) > budget_ns_) return false;
      }
    }
    return true;
  }

private:
  long budget_ns_;
  timespec t0_{};
  unsigned spins_ = 0;
};
template <typename P>
inline bool spin_until(P && pred, long budget_ns)
{
  return SpinBudget(budget_ns).until(pred);
}

}  // namespace mh
