// rt_selftest.h -- launch interface of the device self-tests (rt_selftest.hip), shared with rt_api_query.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/rt_hip.h"
#include "rt_types.h"
#include "rt_sky_tiles.h"

namespace rt {

hipError_t launch_selftest_lean(hipStream_t stream, uint32_t blocks, uint64_t n_per_thread, uint64_t seed, unsigned long long *mismatches);
hipError_t launch_selftest_pair_primary(hipStream_t stream, const DevPairScene &pair, const float root_min[3], const float root_max[3], const float origin[3],
                                        const DevPairPrimary &host_block, unsigned long long *mismatches);

struct DevSkySelftest {
	uint64_t seed;
	uint64_t n;          // streams: sample i runs on rt_rng_seed(seed, 0, i)
	float *out_dirs;     // 3 * n: sky_sample of stream i
	float *out_pdf_s;    // n: sky_pdf at that direction
	const float *dirs;   // 3 * m directions the caller chose
	uint64_t m;
	float *out_pdf;      // m: sky_pdf at each of them
};

// the dynamic LDS the kernel needs with the tables staged (render_kernel's prologue layout: rows, marginal, padding to 16 bytes, guides)
size_t sky_selftest_lds_bytes(const DevScene &S);
hipError_t launch_sky_selftest(bool tables_in_lds, hipStream_t stream, const DevScene &S, const DevSkySelftest &P);


// ---- rt_selftest_forms.hip.  Every launch below adds to counters the caller has set (zeros; all ones in a first-index slot) and runs
// its cases grid-stride (rt_selftest_dev.h); the "in use" reports are the host's to fill in, the kernels leave those words alone. ----

// rt_selftest_short_forms: the device-side counters
constexpr uint32_t kShortFormsRcpExponentCount = 8;
struct DevShortForms {
	unsigned long long *tested;          // [2]: reciprocal inputs, square-root inputs
	unsigned long long *mismatches;      // [RT_SHORT_FORMS]
	unsigned long long *first_index;     // [RT_SHORT_FORMS]: smallest enumeration index that mismatched
	unsigned long long *sqrt_raw;        // [4]: exact, one ulp high, one ulp low, further off
	unsigned long long *site_tested;     // [1]
	unsigned long long *site_mismatches; // [RT_SHORT_SITES]
};
uint32_t short_forms_input_bits(int form, uint64_t index); // the input the enumeration runs at `index`
uint32_t short_forms_in_use();                             // bit k: the render kernels use form k
hipError_t launch_short_forms(hipStream_t stream, const DevShortForms &D, const float *operands, uint64_t n_operands);

// rt_selftest_div_forms (rt_selftest_forms.hip): device pointers; counts zeroed by the caller except the two first indices (all ones)
enum { kDivCountTested = 0, kDivCountBad = 1, kDivCountFirst = 1 + RT_DIV_FORMS, kDivCountSiteTested = 1 + 2 * RT_DIV_FORMS, kDivCountSiteInDomain,
       kDivCountSiteBad, kDivCounts = kDivCountSiteBad + RT_DIV_SITES };
struct DevDivForms {
	const uint32_t *denominators; // or null: first_denominator + j
	uint32_t n_denominators, first_denominator;
	const int32_t *exponents;
	uint32_t n_exponent_pairs;
	unsigned long long *counts; // [kDivCounts]; a first index is (exponent pair * n_denominators + denominator) << 23 | numerator significand
};
uint32_t div_forms_in_use(); // bit k: the render kernels' guarded divisions use form k
hipError_t launch_div_forms(hipStream_t stream, const DevDivForms &D);
hipError_t launch_div_sites(hipStream_t stream, const float *operand_pairs, uint64_t n_pairs, unsigned long long *counts);
hipError_t launch_sky_pdf_forms(hipStream_t stream, const DevScene &S, const float *dirs, uint64_t m, float *out_pair, float *out_default);
// rt_selftest_sky_cell (rt_selftest_forms.hip): cases (su, sv, bits of r_u, bits of r_v), or cases == null: all n = 2^24 jitters of `axis` at (su, sv)
hipError_t launch_sky_cell(hipStream_t stream, const DevScene &S, const DevSkyCell &guard, const uint32_t *cases, uint64_t n, uint32_t *out, unsigned long long *counts, uint32_t axis,
                           uint32_t su, uint32_t sv);
bool sky_cell_in_use(); // rt_lean.h lean_sky_cell(true)

// rt_selftest_frame_forms (rt_selftest_forms.hip): n vectors of 3 floats, counts[RT_FRAME_FORMS_COUNTS] zeroed by the caller (the
// kernel leaves RT_FRAME_FORMS_IN_USE alone: the caller fills it from frame_forms_in_use)
uint32_t frame_forms_in_use(); // bit RT_FRAME_FORM_*: what the two-sphere kernels' switches select (rt_lean.h)
hipError_t launch_frame_forms(hipStream_t stream, const float *vectors, uint64_t n_vectors, unsigned long long *counts);

// rt_selftest_gen_keys (rt_selftest_forms.hip): n cases of RT_GEN_KEYS_CASE_WORDS words on the key table of `seed`, counts[RT_GEN_KEYS_COUNTS]
// zeroed by the caller (the kernel leaves RT_GEN_KEYS_IN_USE alone: the caller fills it from gen_keys_in_use)
uint32_t gen_keys_in_use(); // bit RT_GEN_KEYS_FORM_*: what the two-sphere kernels' switches select (rt_lean.h)
hipError_t launch_gen_keys(hipStream_t stream, uint64_t seed, const uint32_t *cases, uint64_t n_cases, unsigned long long *counts);

// rt_selftest_pair_shadow (rt_selftest_forms.hip): n cases of RT_PAIR_SHADOW_CASE_FLOATS floats, counts[RT_PAIR_SHADOW_COUNTS] zeroed by the caller
hipError_t launch_pair_shadow(hipStream_t stream, const float *cases, uint64_t n_cases, unsigned long long *counts);
// rt_selftest_pair_shadow_walk: n cases of RT_PAIR_SHADOW_WALK_CASE_FLOATS floats, counts[RT_PAIR_SHADOW_WALK_COUNTS] zeroed by the caller
hipError_t launch_pair_shadow_walk(hipStream_t stream, const float *cases, uint64_t n_cases, unsigned long long *counts);

// rt_selftest_sky_tiles (rt_selftest_forms.hip): one byte per tile of the frame, zeroed by the caller
hipError_t launch_sky_tiles(hipStream_t stream, const DevSkyTiles &T, uint32_t width, uint32_t height, uint32_t log2_w, uint32_t tiles_x, uint64_t n_tiles, uint8_t *out);

} // namespace rt
