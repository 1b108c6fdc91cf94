"""The operands tests/test_gpu_div_forms.py (device) and tests/test_div_forms_host.py (CPU model) enumerate the one-pair quotient of
csrc/rt_lean.h over: ONE list, so the two cannot drift apart.  No GPU fixture, no torch."""
import numpy as np

# denominator significands: 1.0, all ones and its neighbours, 1 and 2 ulp above 1, 1.5 -+ 1 ulp, sqrt 2's, 54 from a fixed seed
DENOMINATORS = np.concatenate([
    np.array([0x000000, 0x7FFFFF, 0x7FFFFE, 0x7FFFFD, 0x000001, 0x000002, 0x3FFFFF, 0x400000, 0x400001, 0x3504F3], dtype=np.uint32),
    np.random.default_rng(9).integers(0, 1 << 23, size=54, dtype=np.uint64).astype(np.uint32)])
DENOMINATORS.setflags(write=False)
# (numerator exponent, denominator exponent): (0, 0); the ends of the tame range [2^-81, 2^41] with the exponents less than 96
# apart; and the bounds the call sites test (csrc/rt_shade.h kSitePdf*, kSiteNum*)
EXPONENTS = ((0, 0), (-81, -81), (41, 41), (41, -54), (-54, 41), (-81, 14), (14, -81), (-75, 20), (41, -27))
