// rt_selftest_forms.hip -- rt_selftest_pair_shadow (below) and rt_selftest_short_forms (include/rt_hip.h): the short forms of rt_lean.h that rest on what gfx950's
// v_rcp_f32 / v_sqrt_f32 return, ENUMERATED against the plain operators on the device, and the call sites that guard them on
// operands the caller chooses.  Every kernel is a comparison inside for_each_case with its counters in a Tally, launched by
// launch_cases (rt_selftest_dev.h): integer counters through atomicAdd / atomicMin; no array is indexed by anything but a
// compile-time constant.  A translation unit of its own: tests/test_sky_resources.py pins the kernels of rt_selftest.hip's bundle by name.
#include "rt_shade.h"
#include "rt_gen_keys.h"
#include "rt_selftest.h"
#include "rt_selftest_dev.h"

namespace rt {

// input `index` of the reciprocal enumeration: exponent slot (index >> 24), sign (bit 23), significand (bits 0-22)
__host__ __device__ inline uint32_t short_forms_rcp_input(uint64_t index)
{
	static_assert(kShortFormsRcpExponentCount == 8, "one case per exponent");
	int e = 0;
	switch ((uint32_t)(index >> 24)) { // the ends of rt_lean.h's tame range and between
	case 0: e = -81; break;
	case 1: e = -60; break;
	case 2: e = -24; break;
	case 3: e = -1; break;
	case 4: e = 0; break;
	case 5: e = 1; break;
	case 6: e = 24; break;
	default: e = 41; break;
	}
	return ((uint32_t)(index >> 23) & 1u) << 31 | (uint32_t)(127 + e) << 23 | ((uint32_t)index & 0x007FFFFFu);
}

// (the forms' mismatch counts and first indices, by RT_SHORT_FORM_*; the inputs tested: reciprocals in slot 0, square roots in 1)
using FormTally = Tally<RT_SHORT_FORMS>;
constexpr uint64_t kShortFormsRcpInputs = (uint64_t)kShortFormsRcpExponentCount << 24, kShortFormsSqrtInputs = 1ull << 32;

__global__ __launch_bounds__(256) void short_forms_rcp_kernel(DevShortForms D)
{
	FormTally T;
	Tally<2> tested;
	for_each_case(kShortFormsRcpInputs, [&](uint64_t i) {
		const float d = __uint_as_float(short_forms_rcp_input(i));
		const float want = 1.0f / d;
		T.note(RT_SHORT_FORM_RCP_REFINED, !same_f32(lean_inv_gfx950(d), want), i);
		const float r1 = lean_rcp_refined(d);
		T.note(RT_SHORT_FORM_INV_ONE_PAIR, !same_f32(__builtin_fmaf(__builtin_fmaf(-d, r1, 1.0f), r1, r1), want), i);
		T.note(RT_SHORT_FORM_INV_TWO_PAIRS, !same_f32(lean_inv(d), want), i);
		tested.add(0);
	});
	tested.flush(D.tested);
	T.flush(D.mismatches, D.first_index);
}

// every bit pattern of lean_sqrt's stated domain: all but the positives below 2^-96 (bits 1 .. 0x0F7FFFFF) and the negative
// denormals (0x80000001 .. 0x807FFFFF).  One ulp high means the downward correction is needed somewhere, one ulp low the upward one.
__global__ __launch_bounds__(256) void short_forms_sqrt_kernel(DevShortForms D)
{
	FormTally T;
	Tally<2> tested;
	Tally<4> raw_is; // exact, high, low, other
	for_each_case(kShortFormsSqrtInputs, [&](uint64_t i) {
		const uint32_t bits = (uint32_t)i;
		if ((bits >= 1u && bits < 0x0F800000u) || (bits > 0x80000000u && bits < 0x80800000u))
			return;
		const float x = __uint_as_float(bits);
		const float want = sqrtf(x);
		const float raw = __builtin_amdgcn_sqrtf(x);
		T.note(RT_SHORT_FORM_SQRT_RAW, !same_f32(raw, want), i);
		T.note(RT_SHORT_FORM_SQRT_BOTH, !same_f32(lean_sqrt(x), want), i);
		const uint32_t rb = __float_as_uint(raw), wb = __float_as_uint(want);
		const bool is_exact = same_f32(raw, want);
		const bool is_high = !is_exact && rb == wb + 1u, is_low = !is_exact && rb + 1u == wb; // (positive finite results: bits order as values)
		raw_is.add(0, is_exact);
		raw_is.add(1, is_high);
		raw_is.add(2, is_low);
		raw_is.add(3, !(is_exact || is_high || is_low));
		tested.add(1);
	});
	tested.flush(D.tested);
	raw_is.flush(D.sqrt_raw);
	T.flush(D.mismatches, D.first_index);
}

// the call sites on the caller's operands: each operand as the x, y or z component against tame others, and as all three
template <class F> __device__ __forceinline__ bool ray_new_differs(V3 dir)
{
	const Ray a = ray_new<F>(v3s(0.0f), dir), b = ray_new_plain(v3s(0.0f), dir);
	bool same = same_f32(a.d.x, b.d.x) && same_f32(a.d.y, b.d.y) && same_f32(a.d.z, b.d.z) && same_f32(a.inv.x, b.inv.x) && same_f32(a.inv.y, b.inv.y) &&
	            same_f32(a.inv.z, b.inv.z);
	if (F::tri)
		same = same && same_f32(a.shear.x, b.shear.x) && same_f32(a.shear.y, b.shear.y) && same_f32(a.shear.z, b.shear.z);
	return !same;
}
__global__ __launch_bounds__(256) void short_forms_sites_kernel(DevShortForms D, const float *__restrict__ operands, uint64_t n_operands)
{
	Tally<RT_SHORT_SITES> T;
	Tally<1> tested;
	for_each_case(4u * n_operands, [&](uint64_t i) {
		const float x = operands[i >> 2];
		const uint32_t shape = (uint32_t)i & 3u;
		const V3 dir = shape == 0u ? v3(x, 0.75f, -0.5f) : (shape == 1u ? v3(-0.5f, x, 0.75f) : (shape == 2u ? v3(0.75f, -0.5f, x) : v3(x, x, x)));
		T.add(RT_SHORT_SITE_RAY_NEW_PAIR, ray_new_differs<FeatPair>(dir));
		T.add(RT_SHORT_SITE_RAY_NEW_FULL, ray_new_differs<FeatFull>(dir));
		tested.add(0);
	});
	tested.flush(D.site_tested);
	T.flush(D.site_mismatches);
}

// rt_selftest_pair_shadow: the two-sphere kernels' occlusion predicate for a ray without a limit (rt_intersect.h
// sphere_occludes_unlimited) and the branch-free full test its cold path runs (sphere_occludes_asked), each against
// sphere_t(...) && t > 0 on the caller's cases: centre, radius, origin, direction -- the direction as given, not normalised
__global__ __launch_bounds__(256) void pair_shadow_kernel(const float *__restrict__ cases, uint64_t n_cases, unsigned long long *counts)
{
	Tally<RT_PAIR_SHADOW_COUNTS> T;
	for_each_case(n_cases, [&](uint64_t i) {
		const float *c = cases + i * RT_PAIR_SHADOW_CASE_FLOATS;
		const V3 center = v3(c[0], c[1], c[2]);
		const float radius = c[3];
		Ray r;
		r.o = v3(c[4], c[5], c[6]);
		r.d = v3(c[7], c[8], c[9]);
		r.inv = r.shear = v3s(0.0f); // (no sphere test reads them)
		float t;
		const bool want = sphere_t(center, radius, r, t) && t > 0.0f;
		T.add(RT_PAIR_SHADOW_MISMATCHES, sphere_occludes_unlimited(center, radius, r) != want);
		T.add(RT_PAIR_SHADOW_ASKED_MISMATCHES, sphere_occludes_asked(center, radius, r) != want);
		T.add(RT_PAIR_SHADOW_ASKED, sphere_shadow_signs(center, radius, r).ask);
		T.add(RT_PAIR_SHADOW_TESTED);
	});
	T.flush(counts);
}
hipError_t launch_pair_shadow(hipStream_t stream, const float *cases, uint64_t n_cases, unsigned long long *counts)
{
	return launch_cases(pair_shadow_kernel, stream, n_cases, 2048u, cases, n_cases, counts);
}

// rt_selftest_pair_shadow_walk: trace_any's two-sphere arm AS THE RENDER KERNELS INSTANTIATE IT (FeatPair: sign step, state word,
// cold loop) next to the same arm with the sign step compiled out (the full test of each candidate, as every other limit takes
// it), on a two-sphere scene per case: spheres, their boxes (centre -+ |radius|), ray and `skip` from the caller
struct FeatPairFullShadow : FeatPair {
	static constexpr bool sky_shadows_only = false;
};
constexpr uint32_t kWalkSlot0 = 7u, kWalkSlot1 = 3u; // (any two distinct slots)
__global__ __launch_bounds__(256) void pair_shadow_walk_kernel(const float *__restrict__ cases, uint64_t n_cases, unsigned long long *counts)
{
	Tally<RT_PAIR_SHADOW_WALK_COUNTS> T;
	const DevScene S = {}; // (the two-sphere arm reads neither the scene nor a stack)
	const StackMem M = {};
	for_each_case(n_cases, [&](uint64_t i) {
		const float *c = cases + i * RT_PAIR_SHADOW_WALK_CASE_FLOATS;
		DevPairScene ps = {};
		for (int k = 0; k < 4; ++k) {
			ps.sphere[0][k] = c[k];
			ps.sphere[1][k] = c[4 + k];
		}
		for (int k = 0; k < 3; ++k) {
			ps.c0min[k] = c[k] - fabsf(c[3]); ps.c0max[k] = c[k] + fabsf(c[3]);
			ps.c1min[k] = c[4 + k] - fabsf(c[7]); ps.c1max[k] = c[4 + k] + fabsf(c[7]);
		}
		ps.slot0 = kWalkSlot0;
		ps.slot1 = kWalkSlot1;
		const uint32_t skip = c[14] == 1.0f ? kWalkSlot0 : (c[14] == 2.0f ? kWalkSlot1 : kNoPrim);
		Ray r; // Ray::new with the plain operators (spheres-only: no shear)
		r.o = v3(c[8], c[9], c[10]);
		r.d = v3(c[11], c[12], c[13]);
		r.d = r.d / mag(r.d);
		r.inv = v3(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
		r.shear = v3s(0.0f);
		const float no_limit = __uint_as_float(0x7FC00000u);
		const bool got = trace_any<FeatPair, false>(S, S, M, r, nullptr, no_limit, skip, ps);
		const bool want = trace_any<FeatPairFullShadow, false>(S, S, M, r, nullptr, no_limit, skip, ps);
		T.add(RT_PAIR_SHADOW_WALK_MISMATCHES, got != want);
		// which lanes the sign step sends into the cold loop, and in what state: the arm's own rule, from its own parts
		float tb;
		const bool c0 = aabb_does_int(ps.c0min, ps.c0max, r, tb) && ps.slot0 != skip, c1 = aabb_does_int(ps.c1min, ps.c1max, r, tb) && ps.slot1 != skip;
		const ShadowSigns s0 = sphere_shadow_signs(v3(c[0], c[1], c[2]), c[3], r), s1 = sphere_shadow_signs(v3(c[4], c[5], c[6]), c[7], r);
		const bool occ0 = c0 && s0.occluded, ask0 = c0 && s0.ask;
		const bool occ1 = !occ0 && c1 && s1.occluded, ask1 = !occ0 && c1 && s1.ask;
		T.add(RT_PAIR_SHADOW_WALK_ASKED, ask0 || ask1);
		T.add(RT_PAIR_SHADOW_WALK_ASKED_BOTH, ask0 && ask1);
		T.add(RT_PAIR_SHADOW_WALK_ASKED_WITH_OCCLUDED, (ask0 || ask1) && (occ0 || occ1));
		T.add(RT_PAIR_SHADOW_WALK_TESTED);
	});
	T.flush(counts);
}
hipError_t launch_pair_shadow_walk(hipStream_t stream, const float *cases, uint64_t n_cases, unsigned long long *counts)
{
	return launch_cases(pair_shadow_walk_kernel, stream, n_cases, 2048u, cases, n_cases, counts);
}

// rt_selftest_sky_tiles: the per-tile sky proof (rt_sky_tiles.h) as acquire_coarse asks it -- a wave per tile, lane i testing pixel
// i of the tile and of its eight neighbours, pixels outside the image passing, one ballot -- for every tile of a frame: one byte per tile behind `out`
__global__ __launch_bounds__(256) void sky_tile_flags_kernel(const DevSkyTiles T, uint32_t width, uint32_t height, uint32_t log2_w, uint32_t tiles_x, uint64_t n_tiles,
                                                        uint8_t *__restrict__ out)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint64_t tile = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); tile < n_tiles; tile += (uint64_t)gridDim.x * 4u) { // (wave-uniform)
		const uint32_t ty = (uint32_t)(tile / tiles_x), tx = (uint32_t)(tile - (uint64_t)ty * tiles_x);
		const bool sees_sky = sky_lane_passes(T, tx << log2_w, ty * (64u >> log2_w), log2_w, lane, width, height);
		const unsigned long long bad = __ballot(!sees_sky);
		if (lane == 0u)
			out[tile] = (T.enabled != 0u && bad == 0ull) ? 1u : 0u;
	}
}
hipError_t launch_sky_tiles(hipStream_t stream, const DevSkyTiles &T, uint32_t width, uint32_t height, uint32_t log2_w, uint32_t tiles_x, uint64_t n_tiles, uint8_t *out)
{
	return launch_cases(sky_tile_flags_kernel, stream, n_tiles * 64u, 2048u, T, width, height, log2_w, tiles_x, n_tiles, out);
}

// rt_selftest_div_forms, the enumeration: a work item is one denominator at one exponent pair against 2^kDivChunkBits consecutive
// numerator significands; the refined reciprocal is formed once per item, as a shared-reciprocal site forms it
constexpr uint32_t kDivChunkBits = 10, kDivChunkShift = 23u - kDivChunkBits;
__host__ __device__ inline uint64_t div_forms_items(const DevDivForms &D) { return ((uint64_t)D.n_exponent_pairs * D.n_denominators) << kDivChunkShift; }
__global__ __launch_bounds__(256) void div_forms_kernel(DevDivForms D)
{
	Tally<RT_DIV_FORMS> T;
	Tally<1> tested;
	const uint32_t chunk_shift = kDivChunkShift;
	for_each_case(div_forms_items(D), [&](uint64_t item) {
		const uint64_t pair_index = item >> chunk_shift; // exponent pair * n_denominators + denominator
		const uint32_t chunk = (uint32_t)item & ((1u << chunk_shift) - 1u);
		const uint32_t e = (uint32_t)(pair_index / D.n_denominators), j = (uint32_t)(pair_index - (uint64_t)e * D.n_denominators);
		const uint32_t d_sig = (D.denominators ? D.denominators[j] : D.first_denominator + j) & 0x007FFFFFu;
		const uint32_t n_high = (uint32_t)(127 + D.exponents[2u * e]) << 23;
		const float d = __uint_as_float((uint32_t)(127 + D.exponents[2u * e + 1u]) << 23 | d_sig);
		const float r1 = lean_rcp_refined(d);
		for (uint32_t k = 0; k < (1u << kDivChunkBits); ++k) {
			const uint32_t n_sig = chunk << kDivChunkBits | k;
			const float n = __uint_as_float(n_high | n_sig);
			const float want = n / d;
			const unsigned long long index = pair_index << 23 | n_sig;
			T.note(RT_DIV_FORM_ONE_PAIR, !same_f32(lean_div_core_gfx950(n, d, r1), want), index);
			T.note(RT_DIV_FORM_TWO_PAIRS, !same_f32(lean_div_core(n, d, r1), want), index);
		}
		tested.add(0, 1ull << kDivChunkBits);
	});
	tested.flush(D.counts + kDivCountTested);
	T.flush(D.counts + kDivCountBad, D.counts + kDivCountFirst);
}
hipError_t launch_div_forms(hipStream_t stream, const DevDivForms &D) { return launch_cases(div_forms_kernel, stream, div_forms_items(D), 4096u, D); }
constexpr uint32_t div_form_bit(LeanDivForm f) { return 1u << (f == LeanDivForm::one_pair ? RT_DIV_FORM_ONE_PAIR : RT_DIV_FORM_TWO_PAIRS); }
// from the switch the sites select by (rt_lean.h lean_div_form): only the two-sphere kernels have such sites
uint32_t div_forms_in_use() { return div_form_bit(lean_div_form(true)); }

// ... the wrappers and the guarded sites (rt_shade.h) on the caller's (n, d) pairs.  The plain expressions are kept out of line so
// that nothing is shared with the short forms.
__device__ __noinline__ V3 mis_light_term_plain(V3 te, V3 le, float l_pdf, float m_pdf)
{
	const float a_sq = l_pdf * l_pdf;
	const float mis_weight = a_sq / (a_sq + m_pdf * m_pdf); // power_heuristic (rt_render.hip)
	return te * mis_weight * le / l_pdf;
}
__device__ __noinline__ V3 div3_plain(V3 v, float d) { return v / d; }
__device__ __forceinline__ bool same_v3(V3 a, V3 b) { return same_f32(a.x, b.x) && same_f32(a.y, b.y) && same_f32(a.z, b.z); }
// lean_div_fix's stated domain: d tame, n tame or zero / infinite / NaN, exponents less than 96 apart
__device__ __forceinline__ bool div_fix_domain(float n, float d)
{
	const float an = fabsf(n), ad = fabsf(d);
	const bool d_tame = ad >= 0x1p-81f && ad <= 0x1p41f;
	const bool n_tame = an >= 0x1p-81f && an <= 0x1p41f;
	const int apart = (int)(__float_as_uint(an) >> 23) - (int)(__float_as_uint(ad) >> 23);
	return d_tame && ((n_tame && apart < 96 && apart > -96) || an == 0.0f || an == INFINITY || n != n);
}
__global__ __launch_bounds__(256) void div_sites_kernel(const float *__restrict__ pairs, uint64_t n_pairs, unsigned long long *counts)
{
	Tally<kDivCounts> T; // (the site counters of it)
	for_each_case(n_pairs, [&](uint64_t i) {
		const float n = pairs[2u * i], d = pairs[2u * i + 1u];
		if (div_fix_domain(n, d)) {
			T.add(kDivCountSiteInDomain);
			T.add(kDivCountSiteBad + RT_DIV_SITE_FIX, !same_f32(lean_div_fix_for<true>(n, d), n / d));
			// (a tame, a zero and an infinite neighbour share the reciprocal)
			const V3 v = v3(n, 0.0f, -INFINITY);
			T.add(kDivCountSiteBad + RT_DIV_SITE_DIV3_FIX, !same_v3(lean_div3_fix_for<true>(v, d), div3_plain(v, d)));
		}
		// the light term: (n, d) as (m_pdf, l_pdf) and the other way round, then as a component of te under tame pdfs (the weight is
		// 0.5 there, so 2 n reaches the quotient as n), alone and as all three
		const V3 one = v3s(1.0f), te = v3(1.0f, 0.75f, -0.5f);
		bool ok = same_v3(mis_light_term_short(te, one, d, n), mis_light_term_plain(te, one, d, n));
		ok = ok && same_v3(mis_light_term_short(te, one, n, d), mis_light_term_plain(te, one, n, d));
		const V3 tx = v3(2.0f * n, 0.75f, -0.5f), tz = v3(0.75f, -0.5f, 2.0f * n), ta = v3s(2.0f * n);
		ok = ok && same_v3(mis_light_term_short(tx, one, 1.0f, 1.0f), mis_light_term_plain(tx, one, 1.0f, 1.0f));
		ok = ok && same_v3(mis_light_term_short(tz, one, d, d), mis_light_term_plain(tz, one, d, d));
		ok = ok && same_v3(mis_light_term_short(ta, v3(1.0f, d, -1.0f), 1.0f, 1.0f), mis_light_term_plain(ta, v3(1.0f, d, -1.0f), 1.0f, 1.0f));
		T.add(kDivCountSiteBad + RT_DIV_SITE_MIS_LIGHT_TERM, !ok);
		T.add(kDivCountSiteBad + RT_DIV_SITE_ATAN2,
		      !(same_f32(lean_atan2_for<true>(n, d), lean_atan2(n, d)) && same_f32(lean_atan2_for<true>(d, n), lean_atan2(d, n)) &&
		        same_f32(lean_atan2_for<true>(-n, d), rt_atan2f(-n, d))));
		T.add(kDivCountSiteTested);
	});
	T.flush(counts);
}
hipError_t launch_div_sites(hipStream_t stream, const float *operand_pairs, uint64_t n_pairs, unsigned long long *counts)
{
	return launch_cases(div_sites_kernel, stream, n_pairs, 2048u, operand_pairs, n_pairs, counts);
}

// rt_selftest_sky_pdf_forms: sky_pdf as the two-sphere kernels instantiate it and as every other kernel does, tables in global memory
struct SkyPdfFormsArgs {
	DevScene S;
	const float *dirs;
	uint64_t m;
	float *out_pair, *out_default;
};
__global__ __launch_bounds__(256) void sky_pdf_forms_kernel(const SkyPdfFormsArgs A)
{
	SkyTables T;
	T.row_cdf = A.S.sky.row_cdf;
	T.marginal_cdf = A.S.sky.marginal_cdf;
	T.guide = A.S.sky.guide;
	T.guide_k = A.S.sky.guide_k;
	T.inv_res = nullptr; // (sky_pdf reads none of the verified reciprocals)
	for_each_case(A.m, [&](uint64_t j) {
		const V3 wi = v3(A.dirs[3 * j], A.dirs[3 * j + 1], A.dirs[3 * j + 2]);
		A.out_pair[j] = sky_pdf<true>(A.S, T, wi);
		A.out_default[j] = sky_pdf(A.S, T, wi);
	});
}
hipError_t launch_sky_pdf_forms(hipStream_t stream, const DevScene &S, const float *dirs, uint64_t m, float *out_pair, float *out_default)
{
	SkyPdfFormsArgs A;
	A.S = S;
	A.dirs = dirs;
	A.m = m;
	A.out_pair = out_pair;
	A.out_default = out_default;
	return launch_cases(sky_pdf_forms_kernel, stream, m, 2048u, A);
}

// rt_selftest_sky_cell: the carried sky cell (rt_shade.h sky_direction_<true> -> sky_pdf_carried_, what do_light hands do_scatter in the
// two-sphere kernels) next to sky_pdf<true> at sky_direction_<false>'s direction, tables in global memory, the guard's words read
// through the kernarg pointer as render_kernel reads them.  Consecutive cases are consecutive lanes of a wave: the caller's order
// decides which waves are all guarded, all unguarded or mixed.  cases == null: the enumeration -- case i is jitter i 2^-24 on
// `axis` (0: u, 1: v) of cell (su, sv), the other axis at 0.5.
struct SkyCellSelftestArgs {
	DevScene S;
	DevSkyCell guard;
	const uint32_t *cases; // su, sv, bits of r_u, bits of r_v
	uint64_t n;
	uint32_t *out;         // RT_SKY_CELL_OUT_WORDS per case (cases only)
	unsigned long long *counts;
	uint32_t axis, su, sv;
};
constexpr uint32_t kCellFromInv =
    (uint32_t)((offsetof(SkyCellSelftestArgs, guard) - offsetof(SkyCellSelftestArgs, S) - offsetof(DevScene, sky) - offsetof(DevSky, inv_res_ok)) / 4u);
__global__ __launch_bounds__(256) void sky_cell_kernel(const SkyCellSelftestArgs args_by_value)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const auto *A = (const __attribute__((address_space(4))) SkyCellSelftestArgs *)__builtin_amdgcn_kernarg_segment_ptr();
	(void)args_by_value;
#else
	const SkyCellSelftestArgs *A = &args_by_value;
#endif
	const DevScene S = A->S;
	SkyTables T;
	T.row_cdf = S.sky.row_cdf;
	T.marginal_cdf = S.sky.marginal_cdf;
	T.guide = S.sky.guide;
	T.guide_k = S.sky.guide_k;
	T.inv_res = reinterpret_cast<KWords>(&A->S.sky.inv_res_ok);
	const uint32_t *const cases = A->cases;
	uint32_t *const out = A->out;
	const uint32_t axis = A->axis, su0 = A->su, sv0 = A->sv;
	Tally<RT_SKY_CELL_COUNTS> tally;
	for_each_case(A->n, [&](uint64_t i) {
		uint32_t su = su0, sv = sv0;
		float r_u = 0.5f, r_v = 0.5f;
		if (cases) {
			su = cases[4u * i];
			sv = cases[4u * i + 1u];
			r_u = __uint_as_float(cases[4u * i + 2u]);
			r_v = __uint_as_float(cases[4u * i + 3u]);
		} else {
			(axis == 0u ? r_u : r_v) = (float)(uint32_t)i * 0x1p-24f;
		}
		uint32_t cell, unused;
		const float nu = next_float((float)su + r_u), nv = next_float((float)sv + r_v); // (as sky_sample forms them)
		const V3 d = sky_direction_<true>(T, S.sky.res_x, S.sky.res_y, su, sv, r_u, r_v, nu, nv, cell, kCellFromInv);
		const V3 d_default = sky_direction_<false>(T, S.sky.res_x, S.sky.res_y, su, sv, r_u, r_v, nu, nv, unused);
		uint32_t ui, vi, rx, ry;
		const float got = sky_pdf_carried_(S, T, d, cell, ui, vi);
		const float want = sky_pdf<true>(S, T, d_default);
		const SkyCell c = sky_pdf_cell<true>(S, d_default, rx, ry);
		const bool guarded = (cell >> 31) != 0u, agree = c.ui == su && c.vi == sv;
		tally.add(RT_SKY_CELL_GUARDED_DISAGREE, guarded && !agree);
		tally.add(RT_SKY_CELL_UNGUARDED, !guarded);
		tally.add(RT_SKY_CELL_UNGUARDED_AGREE, !guarded && agree);
		tally.add(RT_SKY_CELL_PDF_MISMATCHES, !same_f32(got, want));
		tally.add(RT_SKY_CELL_TESTED);
		if (cases) {
			uint32_t *o = out + RT_SKY_CELL_OUT_WORDS * i;
			o[0] = __float_as_uint(got);
			o[1] = __float_as_uint(want);
			// (sin_theta <= 0: both pdfs are 0 and neither reads a cell)
			const bool reads = sqrt_unit_(1.0f - d_default.z * d_default.z) > 0.0f;
			o[2] = reads ? ui | vi << 16 | (cell & 0x80000000u) : RT_SKY_CELL_NO_CELL | (cell & 0x80000000u);
			o[3] = reads ? c.ui | c.vi << 16 : RT_SKY_CELL_NO_CELL;
		}
	});
	tally.flush(A->counts);
}
hipError_t launch_sky_cell(hipStream_t stream, const DevScene &S, const DevSkyCell &guard, const uint32_t *cases, uint64_t n, uint32_t *out, unsigned long long *counts, uint32_t axis,
                           uint32_t su, uint32_t sv)
{
	SkyCellSelftestArgs A;
	A.S = S;
	A.guard = guard;
	A.cases = cases;
	A.n = n;
	A.out = out;
	A.counts = counts;
	A.axis = axis;
	A.su = su;
	A.sv = sv;
	return launch_cases(sky_cell_kernel, stream, n, 2048u, A);
}
bool sky_cell_in_use() { return lean_sky_cell(true); }

// rt_selftest_frame_forms: the scatter frame and Ray::new's normalisation as the two-sphere kernels' switches select them
// (rt_lean.h lean_frame_form, lean_ray_norm_short) next to the plain expressions, each vector as a normal and as a direction.
// The plain frame is kept out of line so that nothing is shared with the short form.
__device__ __noinline__ Coord coord_from_z_plain(V3 z) { return coord_from_z(z); }
__device__ __forceinline__ Coord pair_kernels_frame(V3 z)
{
	return lean_frame_form(true) == LeanFrameForm::guarded_short ? coord_from_z_pair(z) : coord_from_z(z);
}
__global__ __launch_bounds__(256) void frame_forms_kernel(const float *__restrict__ vectors, uint64_t n_vectors, unsigned long long *counts)
{
	Tally<RT_FRAME_FORMS_COUNTS> T; // (RT_FRAME_FORMS_IN_USE stays zero: the host's to fill)
	for_each_case(n_vectors, [&](uint64_t i) {
		const V3 v = v3(vectors[3u * i], vectors[3u * i + 1u], vectors[3u * i + 2u]);
		const Coord got = pair_kernels_frame(v), want = coord_from_z_plain(v);
		T.add(RT_FRAME_FORMS_FRAME_MISMATCHES, !(same_v3(got.x, want.x) && same_v3(got.y, want.y) && same_v3(got.z, want.z)));
		const float a = fabsf(v.x) > fabsf(v.y) ? v.x : v.y; // the frame's guard, from its own parts (rt_shade.h)
		T.add(RT_FRAME_FORMS_FRAME_SHORT, frame_guard_(a, v.z, a * a + v.z * v.z));
		const Ray r = ray_new<FeatPair>(v3s(0.0f), v), p = ray_new_plain(v3s(0.0f), v);
		T.add(RT_FRAME_FORMS_RAY_MISMATCHES, !(same_v3(r.d, p.d) && same_v3(r.inv, p.inv)));
		const float m2 = dot(v, v); // ray_new's guard (rt_intersect.h)
		T.add(RT_FRAME_FORMS_RAY_SHORT, fminf(fminf(fabsf(v.x), fabsf(v.y)), fabsf(v.z)) >= 0x1p-60f && m2 >= 0x1p-40f && m2 <= 0x1p40f);
		T.add(RT_FRAME_FORMS_TESTED);
	});
	T.add(RT_FRAME_FORMS_FRAME_PLAIN, T.n[RT_FRAME_FORMS_TESTED] - T.n[RT_FRAME_FORMS_FRAME_SHORT]);
	T.add(RT_FRAME_FORMS_RAY_PLAIN, T.n[RT_FRAME_FORMS_TESTED] - T.n[RT_FRAME_FORMS_RAY_SHORT]);
	T.flush(counts);
}
hipError_t launch_frame_forms(hipStream_t stream, const float *vectors, uint64_t n_vectors, unsigned long long *counts)
{
	return launch_cases(frame_forms_kernel, stream, n_vectors, 2048u, vectors, n_vectors, counts);
}
uint32_t frame_forms_in_use()
{
	return (lean_frame_form(true) == LeanFrameForm::guarded_short ? 1u << RT_FRAME_FORM_FRAME_SHORT : 0u) |
	       (lean_ray_norm_short(true) ? 1u << RT_FRAME_FORM_RAY_NORM_ONE_PAIR : 0u);
}

// rt_selftest_gen_keys: GEN's stream seed from the host's key table (rt_gen_keys.h), in the grouping the render kernels' switch
// selects, without and with the pixel's product formed ahead, next to rt_rng_seed.  The table travels as a kernel argument and is
// read through the kernarg pointer with scalar loads, as render_kernel reads RenderArgs::gen_keys.
struct GenKeysSelftestArgs {
	DevGenKeys keys;
	uint64_t seed;
	const uint32_t *cases;
	uint64_t n_cases;
	unsigned long long *counts;
};
__device__ __forceinline__ bool same_stream(rt_rng a, rt_rng b, bool &draws_differ)
{
	const bool same = a.s0 == b.s0 && a.s1 == b.s1 && a.s2 == b.s2 && a.s3 == b.s3;
	draws_differ = false;
	for (int d = 0; d < 8; ++d)
		draws_differ |= rt_rng_u32(&a) != rt_rng_u32(&b);
	return same;
}
__global__ __launch_bounds__(256) void gen_keys_kernel(const GenKeysSelftestArgs args_by_value)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const auto *A = (const __attribute__((address_space(4))) GenKeysSelftestArgs *)__builtin_amdgcn_kernarg_segment_ptr();
	(void)args_by_value;
#else
	const GenKeysSelftestArgs *A = &args_by_value;
#endif
	constexpr int lead = lean_gen_keys_lead(true);
	const uint64_t seed = A->seed, n_cases = A->n_cases;
	const uint32_t *const cases = A->cases;
	Tally<RT_GEN_KEYS_COUNTS> T; // (RT_GEN_KEYS_IN_USE stays zero: the host's to fill)
	for_each_case(n_cases, [&](uint64_t i) {
		const uint32_t pixel = cases[4u * i], sample_i = cases[4u * i + 1u];
		const uint64_t sample_begin = ((uint64_t)cases[4u * i + 3u] << 32) | cases[4u * i + 2u];
		const uint64_t sample = sample_begin + sample_i; // (wraps, as GEN's sum does)
		rt_rng want, keyed, item;
		rt_rng_seed(&want, seed, (uint64_t)pixel, sample);
		uint32_t hi0, lo0;
		philox_pixel_product(pixel, hi0, lo0);
		rng_seed_keyed<lead>(&keyed, &A->keys, hi0, lo0, sample);
		// ... and with the product formed ahead of the seeding, behind a barrier the optimiser cannot merge the two across
		uint32_t hi0_item, lo0_item;
		philox_pixel_product(pixel, hi0_item, lo0_item);
#if defined(__HIP_DEVICE_COMPILE__)
		asm volatile("" : "+v"(hi0_item), "+v"(lo0_item));
#endif
		rng_seed_keyed<lead>(&item, &A->keys, hi0_item, lo0_item, sample);
		bool draws;
		T.add(RT_GEN_KEYS_STATE_MISMATCHES, !same_stream(keyed, want, draws));
		T.add(RT_GEN_KEYS_DRAW_MISMATCHES, draws);
		T.add(RT_GEN_KEYS_ITEM_STATE_MISMATCHES, !same_stream(item, want, draws));
		T.add(RT_GEN_KEYS_ITEM_DRAW_MISMATCHES, draws);
		T.add(RT_GEN_KEYS_ZERO_BLOCKS, want.s0 == 1u && (want.s1 | want.s2 | want.s3) == 0u); // (the guard's state; a block (1, 0, 0, 0) itself counts too)
		T.add(RT_GEN_KEYS_TESTED);
	});
	T.flush(A->counts);
}
hipError_t launch_gen_keys(hipStream_t stream, uint64_t seed, const uint32_t *cases, uint64_t n_cases, unsigned long long *counts)
{
	GenKeysSelftestArgs A;
	philox_round_keys(seed, A.keys);
	A.seed = seed;
	A.cases = cases;
	A.n_cases = n_cases;
	A.counts = counts;
	return launch_cases(gen_keys_kernel, stream, n_cases, 2048u, A);
}
uint32_t gen_keys_in_use()
{
	return (lean_gen_keys(true) ? 1u << RT_GEN_KEYS_FORM_TABLE : 0u) | (lean_gen_item_product(true) ? 1u << RT_GEN_KEYS_FORM_ITEM_PRODUCT : 0u);
}

uint32_t short_forms_input_bits(int form, uint64_t index)
{
	return form <= RT_SHORT_FORM_INV_TWO_PAIRS ? short_forms_rcp_input(index) : (uint32_t)index;
}
// from the switch the kernels themselves select by (rt_lean.h lean_inv_form, over both values of F::pair); lean_sqrt has one form
constexpr uint32_t short_form_bit(LeanInvForm f)
{
	return 1u << (f == LeanInvForm::refined ? RT_SHORT_FORM_RCP_REFINED : RT_SHORT_FORM_INV_TWO_PAIRS);
}
uint32_t short_forms_in_use()
{
	return short_form_bit(lean_inv_form(true)) | short_form_bit(lean_inv_form(false)) | 1u << RT_SHORT_FORM_SQRT_BOTH;
}

hipError_t launch_short_forms(hipStream_t stream, const DevShortForms &D, const float *operands, uint64_t n_operands)
{
	if (operands)
		return launch_cases(short_forms_sites_kernel, stream, 4u * n_operands, 2048u, D, operands, n_operands);
	if (hipError_t e = launch_cases(short_forms_rcp_kernel, stream, kShortFormsRcpInputs, 2048u, D); e != hipSuccess)
		return e;
	return launch_cases(short_forms_sqrt_kernel, stream, kShortFormsSqrtInputs, 2048u, D);
}

} // namespace rt
