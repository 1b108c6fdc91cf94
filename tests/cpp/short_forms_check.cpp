// short_forms_check.cpp -- the host pass of the short reciprocal / square-root forms of raytracing-rust_amd/csrc/rt_lean.h.
// On the host the forms ARE the plain operators (the device's are built from v_rcp_f32 / v_sqrt_f32 and are enumerated on the
// GPU by rt_selftest_short_forms), so this checks only that the header still compiles for the host and that its host statements
// agree with `1.0f / d` and `sqrtf`.  Built by tests/test_short_forms_host.py with `hipcc --cuda-host-only`.
// Prints one line per check: "<name> <values tested> <mismatches>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdint>
#include "../../raytracing-rust_amd/csrc/rt_lean.h"
#include "check_common.h"


int main()
{
	const uint32_t stride = 4099u; // a prime: ~1 M bit patterns of every class
	unsigned long long n = 0, bad_inv = 0, bad_inv_short = 0, bad_sqrt = 0;
	for (uint64_t u = 0; u < (1ull << 32); u += stride) {
		const float x = f_of((uint32_t)u);
		bad_inv += !same_f32(rt::lean_inv(x), 1.0f / x);
		bad_inv_short += !same_f32(rt::lean_inv_gfx950(x), 1.0f / x);
		bad_sqrt += !same_f32(rt::lean_sqrt(x), std::sqrt(x));
		++n;
	}
	std::printf("lean_inv %llu %llu\n", n, bad_inv);
	std::printf("lean_inv_gfx950 %llu %llu\n", n, bad_inv_short);
	std::printf("lean_sqrt %llu %llu\n", n, bad_sqrt);
	return 0;
}
