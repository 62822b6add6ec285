#!/usr/bin/env python
"""srbh_value_hist divides by a multiply and a shift: v // d == (v * M) >> 32 with M = floor(2^32 / d) + 1 (srbh_value_hist_magic; d == 1
takes v itself).  include/srbh.h gives the argument; this checks all of it on the CPU: every uint16 v against every d in 2..65535,
65 536 x 65 534 cases, with the library's own M.  Prints one line; exits non-zero at the first divisor that fails.

    python tools/check_value_hist_division.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import _lib  # noqa: E402


def main():
    lib = _lib.lib()
    assert lib.srbh_value_hist_magic(1) == 0
    v = np.arange(65536, dtype=np.uint64)[None, :]
    chunk = 128
    for d0 in range(2, 65536, chunk):
        d = np.arange(d0, min(d0 + chunk, 65536), dtype=np.uint64)
        magic = np.array([lib.srbh_value_hist_magic(int(x)) for x in d], dtype=np.uint64)
        assert np.array_equal(magic, np.uint64(2 ** 32) // d + np.uint64(1))
        bad = ((v * magic[:, None]) >> np.uint64(32)) != v // d[:, None]
        if bad.any():
            i, j = np.argwhere(bad)[0]
            print("FAILED: %d // %d" % (j, d[i]))
            return 1
    print("v // d == (v * M) >> 32 for all 65536 values of v and all 65534 divisors d in 2..65535 (M = 2^32 // d + 1); d = 1: M = 0, v itself")
    return 0


if __name__ == "__main__":
    sys.exit(main())
