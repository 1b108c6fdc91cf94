// div_forms_check.cpp -- the CPU model of the one-pair f32 quotient of raytracing-rust_amd/csrc/rt_lean.h (lean_div_core_gfx950):
// WITH a correctly rounded reciprocal r = RN(1 / d) -- what gfx950's refined reciprocal is for every tame d, a fact only the device
// can show (rt_selftest_short_forms) -- q0 = n * r, e = fma(-d, q0, n), q = fma(e, r, q0) is `n / d`.  The host's `/` and fmaf are
// the arithmetic contract's operators, so this checks the sequence itself, not the chip: over the denominators of
// tests/test_gpu_div_forms.py x all 2^23 numerator significands, and over 10^7 seeded random significand pairs.  It also counts how
// often q0 alone differs, to show that the check discriminates.  Built by tests/test_div_forms_host.py with
// `hipcc --cuda-host-only -ffp-contract=off -fsanitize=address,undefined`; the device's instructions are compared by the GPU test.
// Prints one line per operand set: "<name> <quotients> <mismatches of the one-pair sequence> <mismatches of q0 alone>".
#include <cmath>
#include <cstdlib>
#include "check_common.h"

static float one_pair(float n, float d, float r)
{
	const float q0 = n * r;
	const float e = std::fmaf(-d, q0, n);
	return std::fmaf(e, r, q0);
}
struct Tally {
	unsigned long long n = 0, bad = 0, bad_q0 = 0;
	void run(float num, float den)
	{
		const float r = 1.0f / den, want = num / den;
		bad += bits_of(one_pair(num, den, r)) != bits_of(want);
		bad_q0 += bits_of(num * r) != bits_of(want);
		++n;
	}
	void print(const char *name) const { std::printf("%s %llu %llu %llu\n", name, n, bad, bad_q0); }
};

int main(int argc, char **argv)
{
	// the denominators the caller lists (hexadecimal significands), at exponent 0 against every numerator significand at exponent 0
	std::vector<uint32_t> dens;
	for (int k = 1; k < argc; ++k)
		dens.push_back((uint32_t)std::strtoul(argv[k], nullptr, 16) & 0x007FFFFFu);
	Tally listed;
	for (uint32_t d_sig : dens) {
		const float den = f_of(127u << 23 | d_sig);
		for (uint32_t n_sig = 0; n_sig < (1u << 23); ++n_sig)
			listed.run(f_of(127u << 23 | n_sig), den);
	}
	listed.print("listed");
	Tally random;
	uint64_t s = 20240607ull;
	for (int k = 0; k < 10000000; ++k) {
		const uint64_t z = next_u64(s);
		random.run(f_of(127u << 23 | ((uint32_t)z & 0x007FFFFFu)), f_of(127u << 23 | ((uint32_t)(z >> 32) & 0x007FFFFFu)));
	}
	random.print("random");
	return 0;
}
