#!/usr/bin/env python3
"""Device-memory growth over many create / use / destroy cycles of every handle type (hipMemGetInfo before and after; the
allocation cache keeps blocks, so the figure to watch is growth BETWEEN two identical batches of cycles)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from mimosa_amd import capi
from handle_lifetime_worker import make_cycle  # the round tests/test_gpu_handle_lifetime.py::test_nothing_leaks runs

hip = C.CDLL("libamdhip64.so")
def rss_mb():
    import psutil
    return psutil.Process().memory_info().rss / 2**20


def free_mb():
    f, t = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value / 2**20

ctx = capi.Context(0)
# one of every handle type per cycle: map and its copy; factor and clone (linearize, batch, align, score_poses); scan with
# prefetch and deskew; photometric model, frame and factor; radar scan and factor; place database; pose graph; keyframe store
cycle = make_cycle(ctx)

for _ in range(20):
    cycle()
ctx.synchronize()
a, ra = free_mb(), rss_mb()
for _ in range(300):
    cycle()
ctx.synchronize()
b, rb = free_mb(), rss_mb()
for _ in range(300):
    cycle()
ctx.synchronize()
c, rc_ = free_mb(), rss_mb()
print(f"host RSS MB {ra:.1f} -> {rb:.1f} -> {rc_:.1f}")
print(f"free MB after warm-up {a:.1f}, after 300 cycles {b:.1f}, after 600 cycles {c:.1f}; growth per cycle {(b - c) / 300 * 1024:.2f} KB")
assert abs(b - c) < 64, "device memory keeps growing"
assert rc_ - rb < 64, "host memory keeps growing"
print("OK")
