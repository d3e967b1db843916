"""Test infrastructure: fp32 fused multiply-add with ONE rounding, vectorised over numpy arrays, for host
restatements that must match a kernel's v_fma_f32 chain bit for bit (math.fma exists from Python 3.13 only and
takes scalars; exact rational arithmetic per element is far too slow for a few million multiply-adds).

a * b is exact in fp64 (24 x 24 significand bits).  The fp64 sum with c is then rounded TO ODD — the error of
the sum is recovered exactly (Knuth's TwoSum) and an inexact sum with an even last bit moves one ulp towards
the lost part — and rounding that to fp32 gives the correctly rounded a * b + c (a 53-bit round-to-odd followed
by a 24-bit round-to-nearest equals the direct rounding as soon as 53 >= 24 + 2).
test_gather_prefix_host.py holds it to exact rational arithmetic."""
import numpy as np


def fma32(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    t = s - p
    err = (p - (s - t)) + (c64 - t)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, odd, s).astype(np.float32)
