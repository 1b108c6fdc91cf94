"""raytracing-rust_amd/csrc/rt_gen_keys.h on the CPU: the Philox key table the host forms once per render against the keys
rt_philox4x32_10 walks through (seeds 0, 1, all ones, the words at which a round key wraps to exactly 0, a low word that overflows
in the first step), ten keyed rounds against rt_philox4x32_10 on random counters, and the keyed seeding -- without and with the
pixel's product formed ahead -- against rt_rng_seed: state words and the first eight draws, bit for bit, over pixels 0, 1, 2^31,
2^32 - 1, sample indices 0 and 1, sample windows that cross 2^32 and 2^64, random cases, and the one counter whose Philox block is
all zero (tests/cpp/gen_keys_check.cpp).  A stand-alone program, its host code built with AddressSanitizer and UBSan.  The device's
instructions are compared by tests/test_gpu_gen_keys.py; rt_philox_round_keys, the library's own table, is checked here too."""
import numpy as np

import host_check

SEEDS = (0, 1, 0xFFFFFFFFFFFFFFFF, 0x61C8864700000000, 0x0000000061C88647, 0x4498517B00000000, 0x12345678F0000000, 0x806AB30FD9C60ABE)


def test_the_key_table_and_the_keyed_seed_are_rt_rng_seed_on_the_host(tmp_path):
    res = host_check.run(host_check.build("gen_keys_check", tmp_path, sanitize=True), timeout=600)
    print(res)
    assert set(res) == {"table", "rounds", "keyed", "item", "zero_block"}
    assert res["table"] == (len(SEEDS) * 20 + 3, 0), res
    assert res["rounds"] == (len(SEEDS) * 20000, 0), res
    per_seed = 4 * 2 * 8 + 20000
    assert res["keyed"] == (len(SEEDS) * per_seed, 0) and res["item"] == (len(SEEDS) * per_seed, 0), res
    assert res["zero_block"] == (1, 0, 1), res  # the block is all zero, every form agrees, and the guard's state came out


def walked_keys(seed):
    """the keys rt_philox4x32_10 xors in, round by round: its own `k0 += 0x9E3779B9; k1 += 0xBB67AE85` on 32-bit words"""
    k0, k1, rows = seed & 0xFFFFFFFF, seed >> 32, []
    for _ in range(10):
        rows.append((k0, k1))
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.array(rows, dtype=np.uint32)


def test_the_librarys_table_is_the_walked_keys(hb):
    for seed in SEEDS:
        assert np.array_equal(hb.philox_round_keys(seed), walked_keys(seed)), hex(seed)
    assert hb.philox_round_keys(0x0000000061C88647)[1, 0] == 0 and hb.philox_round_keys(0x4498517B00000000)[1, 1] == 0
