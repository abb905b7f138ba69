"""Reduces a rocprofv3 kernel trace of tools/icp_align_time.py to the per-kernel table in profiles/icp_align_kernel_stats.txt.

  rocprofv3 --kernel-trace --stats -d OUT -o align -- python tools/icp_align_time.py --one 24576 --repeats 20
  python tools/icp_align_kernel_stats.py OUT/align_results.db > profiles/icp_align_kernel_stats.txt

Reads the `kernels` view of the rocpd database rocprofv3 writes (name, start, end in ns): calls, mean, min and max duration per
kernel, ordered by total time."""
import sqlite3
import sys


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                      "order by sum(end - start) desc").fetchall()
    print("kernel-trace summary of: python tools/icp_align_time.py --one 24576 --repeats 20 (rocprofv3 --kernel-trace; durations in ns)")
    print("%-100s %8s %10s %10s %10s" % ("kernel", "calls", "avg", "min", "max"))
    for name, calls, avg, lo, hi in rows:
        print("%-100s %8d %10.0f %10d %10d" % (name[:100], calls, avg, lo, hi))


if __name__ == "__main__":
    main()
