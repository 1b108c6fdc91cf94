// rt_gen_keys.h -- the stream seed of GEN as the two-sphere kernels form it: rt_rng_seed (include/rt_detmath.h) with the work that
// does not depend on the sample taken out of the per-sample path.  rt_rng_seed itself is untouched -- the host and every other
// kernel seed through it -- and what is here returns its four state words bit for bit, for every (seed, pixel, sample):
//   * the Philox round keys depend on the seed alone: the host forms the table once per render (philox_round_keys) and the kernel
//     reads it with scalar loads (rt_types.h DevGenKeys; switch lean_gen_keys of rt_lean.h).  In the parent's code every key is
//     ONE s_add_i32 of a literal to the seed's word, eighteen per sample; the xors fold the key as their scalar operand either way
//     (gfx950 has no three-way xor: `hi ^ c ^ k` is two v_xor_b32, with a computed key as with a loaded one);
//   * the first round's product 0xD2511F53 * c[0] depends on the pixel alone (c[0] is the pixel's index, whose high word is zero
//     by type here): a lane can form it when it is handed its item and carry the two words (switch lean_gen_item_product).
// rt_selftest_gen_keys runs both forms next to rt_rng_seed on the device; tests/cpp/gen_keys_check.cpp runs them on the host.
#pragma once

#include "rt_types.h"
#include "rt_lean.h"

namespace rt {

// the key schedule of rt_philox4x32_10 for `seed`, with its own wrapping 32-bit adds
RT_FN void philox_round_keys(uint64_t seed, DevGenKeys &K)
{
	uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
	for (int r = 0; r < 10; ++r) {
		K.key[r][0] = k0;
		K.key[r][1] = k1;
		k0 += 0x9E3779B9u;
		k1 += 0xBB67AE85u;
	}
	for (int i = 0; i < 12; ++i)
		K.pad[i] = 0u;
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) DevGenKeys *GenKeysPtr; // kernel arguments: constant memory, scalar loads
#else
typedef const DevGenKeys *GenKeysPtr;
#endif

// The table's address again, usable only once `after` is known: the scalar loads made through the result are issued there, next to
// the rounds that use them, and their registers are not held from the top of GEN.
RT_FN GenKeysPtr gen_keys_after_(GenKeysPtr p, uint32_t after)
{
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("" : "+s"(p) : "v"(after));
#else
	(void)after;
#endif
	return p;
}

// the product of the first round that depends on the pixel alone: (hi, lo) of 0xD2511F53 * pixel
RT_FN void philox_pixel_product(uint32_t pixel, uint32_t &hi0, uint32_t &lo0)
{
	const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)pixel;
	hi0 = (uint32_t)(p0 >> 32);
	lo0 = (uint32_t)p0;
}

// one round of rt_philox4x32_10 under the key given
RT_FN void philox_round_keyed(uint32_t c[4], uint32_t k0, uint32_t k1)
{
	const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c[0];
	const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c[2];
	const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
	const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
	const uint32_t n0 = hi1 ^ c[1] ^ k0;
	const uint32_t n2 = hi0 ^ c[3] ^ k1;
	c[0] = n0;
	c[1] = lo1;
	c[2] = n2;
	c[3] = lo0;
}

// rt_rng_seed(r, seed, pixel, sample) for the seed whose table K is, the pixel whose product (hi0, lo0) is (philox_pixel_product)
// and a pixel index below 2^32.  LEAD = 0: the keys are read in one round of loads wherever the compiler puts them; LEAD = n > 0:
// in three groups (rounds 0 - 3, 4 - 7, 8 - 9), the second and third issued n rounds ahead of their first use, no earlier.
template <int LEAD> RT_FN void rng_seed_keyed(rt_rng *r, GenKeysPtr K, uint32_t hi0, uint32_t lo0, uint64_t sample)
{
	static_assert(LEAD >= 0 && LEAD <= 3, "a group is issued at most three rounds ahead");
	uint32_t c[4];
	GenKeysPtr K1 = K, K2 = K;
	// round 0, on c = (pixel, 0, sample, sample >> 32): its first product is the caller's
	{
		const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)(uint32_t)sample;
		c[0] = (uint32_t)(p1 >> 32) ^ K->key[0][0];
		c[1] = (uint32_t)p1;
		c[2] = hi0 ^ (uint32_t)(sample >> 32) ^ K->key[0][1];
		c[3] = lo0;
	}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int round = 1; round < 10; ++round) {
		if (LEAD > 0 && round == 4 - LEAD)
			K1 = gen_keys_after_(K, c[1]);
		if (LEAD > 0 && round == 8 - LEAD)
			K2 = gen_keys_after_(K, c[1]);
		const GenKeysPtr Kr = round < 4 ? K : (round < 8 ? K1 : K2);
		philox_round_keyed(c, Kr->key[round][0], Kr->key[round][1]);
	}
	if ((c[0] | c[1] | c[2] | c[3]) == 0u)
		c[0] = 1u; /* xoshiro must not start from the all-zero state */
	r->s0 = c[0];
	r->s1 = c[1];
	r->s2 = c[2];
	r->s3 = c[3];
}

} // namespace rt
