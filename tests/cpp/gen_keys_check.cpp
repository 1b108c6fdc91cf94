// gen_keys_check.cpp -- the stream seed of GEN as the coarse two-sphere kernels form it (raytracing-rust_amd/csrc/rt_gen_keys.h) on
// the host: the key table philox_round_keys forms for a seed against the keys rt_philox4x32_10 (include/rt_detmath.h) walks through,
// and the keyed seeding, without and with the pixel's product formed ahead, against rt_rng_seed, bit for bit.  The device's
// instructions are compared by tests/test_gpu_gen_keys.py.  Built by tests/test_gen_keys_host.py with
// `hipcc --cuda-host-only -fsanitize=address,undefined`.
// Prints one line per check: "<name> <cases> <mismatches>", and "zero_block <cases> <mismatches> <guard states seen>".
#include "../../raytracing-rust_amd/csrc/rt_gen_keys.h"
#include "check_common.h"

// what rt_philox4x32_10 xors in at round r, restated without its loop: the seed's word plus r times the Weyl constant, mod 2^32
static uint32_t walked_key(uint32_t word, uint32_t weyl, int r) { return (uint32_t)(((uint64_t)word + (uint64_t)r * weyl) & 0xFFFFFFFFull); }

static uint64_t next_u64() { return next_u64(g_state); }

static bool same(const rt_rng &a, const rt_rng &b) { return a.s0 == b.s0 && a.s1 == b.s1 && a.s2 == b.s2 && a.s3 == b.s3; }
static bool same_draws(rt_rng a, rt_rng b)
{
	bool ok = true;
	for (int d = 0; d < 8; ++d)
		ok = ok && rt_rng_u32(&a) == rt_rng_u32(&b);
	return ok;
}

int main()
{
	// 0 and 1; all ones; a high word and a low word of 2^32 - 0x9E3779B9 (the low one makes k0 wrap to exactly 0 after the first
	// round); the high word that makes k1 wrap to exactly 0; a low word that makes k0 overflow in the first step; and the seed of
	// the all-zero block below
	const uint64_t seeds[] = {0ull, 1ull, 0xFFFFFFFFFFFFFFFFull, 0x61C8864700000000ull, 0x0000000061C88647ull, 0x4498517B00000000ull,
	                          0x12345678F0000000ull, 0x806AB30FD9C60ABEull};
	unsigned long long n = 0, bad = 0;
	for (uint64_t seed : seeds) {
		rt::DevGenKeys K;
		rt::philox_round_keys(seed, K);
		for (int r = 0; r < 10; ++r) {
			bad += K.key[r][0] != walked_key((uint32_t)seed, 0x9E3779B9u, r);
			bad += K.key[r][1] != walked_key((uint32_t)(seed >> 32), 0xBB67AE85u, r);
			n += 2;
		}
	}
	{ // the wraps the seeds were chosen for
		rt::DevGenKeys K;
		rt::philox_round_keys(0x0000000061C88647ull, K);
		bad += K.key[1][0] != 0u;
		rt::philox_round_keys(0x4498517B00000000ull, K);
		bad += K.key[1][1] != 0u;
		rt::philox_round_keys(0x12345678F0000000ull, K);
		bad += !(K.key[1][0] < K.key[0][0]);
		n += 3;
	}
	std::printf("table %llu %llu\n", n, bad);

	// ten keyed rounds on the table are rt_philox4x32_10, for any counter (all four words random)
	n = bad = 0;
	for (uint64_t seed : seeds) {
		rt::DevGenKeys K;
		rt::philox_round_keys(seed, K);
		for (int i = 0; i < 20000; ++i) {
			const uint64_t a = next_u64(), b = next_u64();
			uint32_t c[4] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)}, w[4] = {c[0], c[1], c[2], c[3]};
			for (int r = 0; r < 10; ++r)
				rt::philox_round_keyed(c, K.key[r][0], K.key[r][1]);
			rt_philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
			bad += !(c[0] == w[0] && c[1] == w[1] && c[2] == w[2] && c[3] == w[3]);
			++n;
		}
	}
	std::printf("rounds %llu %llu\n", n, bad);

	// the seeding: seeds x pixels x sample indices x sample windows whose sum with the index crosses 2^32 and 2^64, then random ones
	const uint32_t pixels[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
	const uint64_t begins[] = {0ull, 5ull, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull, 0x8000000000000000ull, 0xDEADBEEFFFFFFFFFull,
	                           0xFFFFFFFFFFFFFFFFull};
	unsigned long long bad_keyed = 0, bad_item = 0;
	n = 0;
	auto run = [&](const rt::DevGenKeys &K, uint64_t seed, uint32_t pixel, uint64_t sample) -> rt_rng {
		rt_rng want, keyed, grouped, item;
		rt_rng_seed(&want, seed, (uint64_t)pixel, sample);
		uint32_t hi0, lo0;
		rt::philox_pixel_product(pixel, hi0, lo0);
		rt::rng_seed_keyed<0>(&keyed, &K, hi0, lo0, sample);
		rt::rng_seed_keyed<2>(&grouped, &K, hi0, lo0, sample);
		const uint64_t p = (uint64_t)0xD2511F53u * (uint64_t)pixel; // the product as the hand-out forms it, restated
		rt::rng_seed_keyed<0>(&item, &K, (uint32_t)(p >> 32), (uint32_t)p, sample);
		bad_keyed += !(same(keyed, want) && same_draws(keyed, want) && same(grouped, want));
		bad_item += !(same(item, want) && same_draws(item, want));
		++n;
		return want;
	};
	for (uint64_t seed : seeds) {
		rt::DevGenKeys K;
		rt::philox_round_keys(seed, K);
		for (uint32_t pixel : pixels)
			for (uint32_t sample_i = 0; sample_i < 2u; ++sample_i)
				for (uint64_t begin : begins)
					run(K, seed, pixel, begin + sample_i);
		for (int i = 0; i < 20000; ++i)
			run(K, seed, (uint32_t)next_u64(), next_u64());
	}
	std::printf("keyed %llu %llu\n", n, bad_keyed);
	std::printf("item %llu %llu\n", n, bad_item);

	// the one counter with pixel < 2^32 whose block is all zero under this seed (found by inverting the ten rounds from the zero
	// block, seed after seed, until the counter's second word came out zero): the guard gives xoshiro (1, 0, 0, 0)
	{
		n = 0;
		bad_keyed = bad_item = 0;
		rt::DevGenKeys K;
		rt::philox_round_keys(0x806AB30FD9C60ABEull, K);
		uint32_t w[4] = {0x1CCED5BFu, 0u, 0xD52EC01Bu, 0xA2047F57u};
		rt_philox4x32_10(w, 0xD9C60ABEu, 0x806AB30Fu);
		const bool block_is_zero = (w[0] | w[1] | w[2] | w[3]) == 0u;
		const rt_rng got = run(K, 0x806AB30FD9C60ABEull, 0x1CCED5BFu, 0xA2047F57D52EC01Bull);
		const bool guarded = got.s0 == 1u && (got.s1 | got.s2 | got.s3) == 0u;
		std::printf("zero_block %llu %llu %d\n", n, bad_keyed + bad_item + (block_is_zero ? 0ull : 1ull), guarded ? 1 : 0);
	}
	return 0;
}
