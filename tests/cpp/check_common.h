// check_common.h -- what the stand-alone host checks of this directory share: the bit casts, the bit-for-bit comparisons, the seeded
// operand generator and the writer of a case table.  HIP-free and header-only; a check program includes it next to the header it tests.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static inline uint32_t bits_of(float f)
{
	uint32_t b;
	std::memcpy(&b, &f, sizeof b);
	return b;
}
static inline float f_of(uint32_t u)
{
	float f;
	std::memcpy(&f, &u, sizeof f);
	return f;
}
static inline bool same_f32(float a, float b) { return bits_of(a) == bits_of(b) || (a != a && b != b); } // any NaN equals any NaN
template <class V3> static inline bool same_v3(const V3 &a, const V3 &b) { return same_f32(a.x, b.x) && same_f32(a.y, b.y) && same_f32(a.z, b.z); }

// one 64-bit LCG step and a mix, seeded; enough for operands.  next_u32 is the generator of the programs that keep one global
// stream: bits 16..47 of the mixed word
static inline uint64_t next_u64(uint64_t &state)
{
	state = state * 6364136223846793005ull + 1442695040888963407ull;
	uint64_t x = state;
	x ^= x >> 33;
	x *= 0xFF51AFD7ED558CCDull;
	x ^= x >> 33;
	return x;
}
inline uint64_t g_state = 0x9E3779B97F4A7C15ull;
static inline uint32_t next_u32() { return (uint32_t)(next_u64(g_state) >> 16); }
static inline float unit() { return (float)(next_u32() >> 8) * 0x1p-24f; } // [0, 1)
static inline float signed_unit() { return 2.0f * unit() - 1.0f; }         // [-1, 1)

// the cases a check ran, as raw floats, for the device self-test to run the very same operands; 0, or 1 with a message
static inline int write_cases(const char *path, const std::vector<float> &cases)
{
	std::FILE *f = std::fopen(path, "wb");
	if (!f || std::fwrite(cases.data(), sizeof(float), cases.size(), f) != cases.size() || std::fclose(f) != 0) {
		std::fprintf(stderr, "cannot write %s\n", path);
		return 1;
	}
	return 0;
}
