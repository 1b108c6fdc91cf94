// rt_lean.h -- the SAME f32 results as include/rt_detmath.h and the IEEE operators, in fewer gfx950 instructions.
//
// The arithmetic contract (rt_detmath.h + correctly rounded +,-,*,/,sqrt) fixes WHAT every operation returns.  How hipcc
// gets there is expensive on this chip, and a third of the render kernels' vector instructions is spent on it:
//   * `a / b`       11 instructions: v_div_scale x2, v_rcp, 2 fma (reciprocal refinement), mul + 4 fma (quotient with two
//                   corrections), v_div_fmas, v_div_fixup;
//   * `sqrtf(x)`    16: a 2^32 pre-scale for tiny inputs, v_sqrt, two one-ulp corrections, the un-scale, a class fix-up;
//   * rt_sinf / rt_cosf / rt_acosf / rt_atan2f compile to DIVERGENT branches: both polynomial kernels run in turn
//     whenever the lanes of a wave disagree (they always do), sin and cos of one angle reduce the argument twice, and the
//     guards of the huge-argument paths are paid on every call.
// This header restates them so that the instructions which cannot change the result are not executed:
//   * lean_sincos / lean_acos / lean_atan2: the operations of rt_detmath.h on every input of their stated domain, one
//     polynomial evaluation per result, selects instead of branches.  Plain C++ over +,-,*,/,sqrt,fmaf: they compile on
//     the host too, where tests/test_lean_math.py checks them against rt_detmath.h bit for bit (exhaustively over the
//     float ranges the render path feeds them);
//   * lean_div* / lean_sqrt (device only): hipcc's own expansion MINUS the steps that are the identity on "tame" operands.
//     v_div_scale_f32 returns its operand unchanged and clears VCC unless an operand is zero / denormal / the quotient or
//     the reciprocal would leave the normal range (exponent differences >= 96 or <= -126, numerator below 2^-103);
//     v_div_fmas_f32 with VCC clear is v_fma_f32; v_div_fixup_f32 returns the quotient unchanged unless an operand is
//     zero, infinite or NaN or the exponents differ by more than the format allows.  So for operands whose magnitudes lie
//     in [2^-81, 2^41] and whose exponent difference stays below 96 the remaining instructions compute bit for bit what
//     `a / b` computes.  Every use states why its operands are tame, or tests it (one or two compares per ray) and takes
//     the plain operator otherwise.  rt_selftest_lean (rt_api_query.cpp) runs both forms side by side ON THE DEVICE over random
//     and edge-case operands; tests/test_gpu_parity.py::test_lean_arithmetic_matches_the_ieee_operators asserts zero
//     mismatches, and every parity test compares frames that went through them with the CPU checker's plain C.
#pragma once

#include "rt_vec.h"

namespace rt {

// ---- branch-free restatements of rt_detmath.h (host + device) ----

// (rt_sinf(x), rt_cosf(x)) for |x| <= 2^22 (rt_reduce_pio2's Cody-Waite range; finite, so neither the NaN guard nor the
// binary64 fold of rt_detmath.h can trigger).  Callers: angles 2*pi*r and pi*v with r, v in [0, 1 + 2^-20].
RT_FN void lean_sincos(float x, float &s, float &c)
{
	const float k = rintf(x * 0.636619746685028076172f);
	float r = fmaf(-k, 1.57079637050628662109f, x);
	r = fmaf(-k, -4.37113882867379282984e-08f, r);
	r = fmaf(-k, -1.71512451000588185479e-15f, r);
	const int q = (int)k;
	const float sk = rt_sin_kernel(r), ck = rt_cos_kernel(r);
	const bool odd = (q & 1) != 0;
	const float sv = odd ? ck : sk;
	const float cv = odd ? sk : ck;
	s = (q & 2) ? -sv : sv;
	c = ((q + 1) & 2) ? -cv : cv;
}

// rt_acosf(x) for every x (NaN and |x| > 1 give NaN there and here): 1 + x == 1 - |x| for x < 0, so the two outer arms
// share one square root and all three share one polynomial.
RT_FN float lean_acos_with(float x, float sqrt_half_one_minus_abs)
{
	const bool big = fabsf(x) > 0.5f;
	const float k = rt_asin_kernel(big ? sqrt_half_one_minus_abs : x);
	const float two_k = 2.0f * k;
	return big ? (x > 0.0f ? two_k : RT_PI - two_k) : RT_FRAC_PI_2 - k;
}
RT_FN float lean_acos(float x) { return lean_acos_with(x, sqrtf(0.5f * (1.0f - fabsf(x)))); }

// rt_atan_unit(t) for t in [0, 1] given q = (t - 1) / (t + 1) (used only where t > tan(pi/8))
RT_FN float lean_atan_unit_with(float t, float q)
{
	const bool upper = t > 0.414213567972183227539f;
	const float u = upper ? q : t;
	const float z = u * u;
	float p = fmaf(8.05374449538e-2f, z, -1.38776856032e-1f);
	p = fmaf(p, z, 1.99777106478e-1f);
	p = fmaf(p, z, -3.33329491539e-1f);
	return (upper ? RT_FRAC_PI_4 : 0.0f) + fmaf(p * z, u, u);
}
// rt_atan2f(y, x) for every (y, x): the quotient min/max is the quotient the taken arm of rt_atan2f forms
template <class DivA, class DivB> RT_FN float lean_atan2_with(float y, float x, DivA div_ratio, DivB div_octant)
{
	const float ax = fabsf(x), ay = fabsf(y);
	const bool swap = ay > ax;
	const float t = div_ratio(swap ? ax : ay, swap ? ay : ax);
	const float a = lean_atan_unit_with(t, div_octant(t - 1.0f, t + 1.0f));
	float r = swap ? RT_FRAC_PI_2 - a : a;
	r = (ax == ay) ? RT_FRAC_PI_4 : r;
	r = (ax == 0.0f && ay == 0.0f) ? 0.0f : r;
	if (rt_f32_bits(x) & 0x80000000u)
		r = RT_PI - r;
	r = (rt_f32_bits(y) & 0x80000000u) ? -r : r;
	return (x != x || y != y) ? x + y : r;
}
RT_FN float lean_atan2_portable(float y, float x)
{
	return lean_atan2_with(y, x, [](float n, float d) { return n / d; }, [](float n, float d) { return n / d; });
}

// ---- x / c for a divisor the launch knows beforehand, c in [2^-20, 2^32], rc = RN(1 / c) formed on the host, which has also
// VERIFIED (rt_build.cpp verified_reciprocal: every one of the 2^23 significands of x) that these three IEEE operations return the
// correctly rounded quotient.  The sequence is scale-invariant while nothing under- or overflows, so it holds for x = 0, NaN
// and 2^-60 <= |x| <= 2^60 (x = -0 comes back as +0 where the division returns -0: no use below feeds a -0 whose sign could
// reach a pixel); each use says why its x is in that set (or tests it).  Three plain instructions instead of eleven
// with a v_rcp_f32 among them: 7.5 issue cycles instead of 33 (profiles/r04_valu_issue.txt). ----
RT_FN float div_by_verified(float x, float c, float rc)
{
	const float q0 = x * rc;
	const float e = fmaf(-c, q0, x);
	return fmaf(e, rc, q0);
}
// the two constants the shading code divides by: verified like any other (tests/test_lean_math.py asks the library), their
// reciprocals are the compile-time IEEE quotients
constexpr float kRcpPi = 1.0f / RT_PI, kRcpTau = 1.0f / RT_TAU;

// which form of 1 / d Ray::new takes (lean_inv_for below): the two-sphere kernels the reciprocal proven for gfx950, the others keep
// lean_inv, instruction for instruction (they sit on guarded register budgets, tests/test_resource_table.py, and have not been
// measured with it).  lean_inv_for selects by this and rt_selftest_short_forms reports its forms "in use" from it (rt_selftest_forms.hip
// short_forms_in_use), so a kernel moved to another form here is a form the enumeration test then asks zero mismatches of.
enum class LeanInvForm { two_pairs, refined };
constexpr LeanInvForm lean_inv_form(bool pair) { return pair ? LeanInvForm::refined : LeanInvForm::two_pairs; }
// ... and which form of n / d the bounce path's guarded divisions take: the two-sphere kernels the quotient with ONE correction
// pair, proven for gfx950 by rt_selftest_div_forms -- lean_div_for and lean_div3_for (no fixup: the test sends zeros to the plain
// operator) at the light-sampling term (rt_shade.h mis_light_term_short), lean_div_fix_for in atan2's octant fold (lean_atan2_for);
// lean_div3_fix_for completes the set and is reached by the self-test alone.  The other kernels are not asked -- their sites keep
// the plain operator, and lean_div* keeps its two pairs wherever it is used today.
// rt_selftest_div_forms reports the form "in use" from this switch (rt_selftest_forms.hip div_forms_in_use).
enum class LeanDivForm { two_pairs, one_pair };
constexpr LeanDivForm lean_div_form(bool pair) { return pair ? LeanDivForm::one_pair : LeanDivForm::two_pairs; }
// ... and two more sites of the two-sphere kernels, each a switch of its own so that each can be built and measured alone
// (-DRT_PAIR_RAY_NORM_SHORT=0 / -DRT_PAIR_FRAME_SHORT=0 put a site back on its previous form; these kernels sit on a scheduling
// knife edge, DESIGN section 4, so a site ships only on its own measured gain):
//   lean_ray_norm_short   Ray::new's normalisation direction / |direction| (rt_intersect.h ray_new, inside the guard it already
//                         has) through lean_div3_for<true>: the one-pair quotient instead of lean_div3's two pairs;
//   lean_frame_form       the scatter frame of a Lambertian bounce (rt_shade.h coord_from_z_pair): the arm chosen once by selects
//                         on the operands, one guard, the short square root, one refined reciprocal and two one-pair quotients;
//                         lanes that fail the guard run the plain expression.
// rt_selftest_frame_forms reports both from these switches (rt_selftest_forms.hip frame_forms_in_use).
// Measured, six interleaved runs each on rtweekend1 (profiles/r10_frame_forms_ab.log; the gate: every run below every parent run and
// a mean gain of three parent spreads): the frame alone -0.819 ms = 6.0 spreads: ON.  The normalisation alone -0.369 ms = 2.7
// spreads, and -0.447 ms on top of the frame = 2.8 of that build's spreads: every run below, but short of the gate both times: OFF,
// ray_new keeps lean_div3 (HISTORY.md).
// Round 25 measured the normalisation again once the parent's spread had tightened (profiles/r25_gen_keys_ab.log, the same gate):
// every run below every run of the build without it and a mean gain of more than three of that build's spreads: ON.
#ifndef RT_PAIR_RAY_NORM_SHORT
#define RT_PAIR_RAY_NORM_SHORT 1
#endif
#ifndef RT_PAIR_FRAME_SHORT
#define RT_PAIR_FRAME_SHORT 1
#endif
constexpr bool lean_ray_norm_short(bool pair) { return pair && RT_PAIR_RAY_NORM_SHORT != 0; }
enum class LeanFrameForm { plain, guarded_short };
constexpr LeanFrameForm lean_frame_form(bool pair) { return pair && RT_PAIR_FRAME_SHORT != 0 ? LeanFrameForm::guarded_short : LeanFrameForm::plain; }
// ... and two switches for the integer work of GEN's stream seed in the coarse two-sphere kernels (rt_gen_keys.h; the same bits as
// rt_rng_seed for every input, rt_selftest_gen_keys):
//   lean_gen_keys           the Philox round keys read from the kernel arguments (rt_types.h DevGenKeys, formed by the host once per
//                           render) instead of eighteen scalar adds per sample.  RT_PAIR_GEN_KEYS: 0 = off (rt_rng_seed); 1 = one
//                           round of loads where the compiler puts them; 2 / 3 / 4 = three groups, the later ones issued 1 / 2 / 3
//                           rounds ahead of their use;
//   lean_gen_item_product   the first round's product 0xD2511F53 * pixel formed when the lane is handed its item and carried in two
//                           registers of lane state (which replace the pixel's index there); needs lean_gen_keys.
// Measured, six interleaved runs each on rtweekend1 against the parent (51.363 - 51.465 ms kernel time, spread 0.102;
// profiles/r25_gen_keys_ab.log): the table in one round of loads +0.027 ms, in three groups two rounds ahead -0.031 ms -- the
// eighteen s_add_i32 are gone from the assembly and the time does not move: both OFF, GEN seeds through rt_rng_seed.  The table
// with the product carried -0.084 ms (0.16 %, 77 VGPRs instead of 76), runs on both sides of the parent's: OFF.
#ifndef RT_PAIR_GEN_KEYS
#define RT_PAIR_GEN_KEYS 0
#endif
#ifndef RT_PAIR_GEN_ITEM_PRODUCT
#define RT_PAIR_GEN_ITEM_PRODUCT 0
#endif
constexpr bool lean_gen_keys(bool pair) { return pair && RT_PAIR_GEN_KEYS != 0; }
constexpr int lean_gen_keys_lead(bool pair) { return lean_gen_keys(pair) ? RT_PAIR_GEN_KEYS - 1 : 0; }
constexpr bool lean_gen_item_product(bool pair) { return lean_gen_keys(pair) && RT_PAIR_GEN_ITEM_PRODUCT != 0; }
// ... and one for the sky pdf of the direction LIGHT sampled itself (rt_shade.h sky_sample_cell / sky_pdf_carried): the table cell
// travels from do_light to do_scatter in one word, and lanes a host-proven guard puts safely inside their cell skip the
// acos / atan2 round trip that would only find it again.  -DRT_PAIR_SKY_CELL=0 compiles it out: do_light and do_scatter are then
// sky_sample and sky_pdf<true>, as before.  Measured: profiles/r27_sky_cell_ab.log, HISTORY.md.
#ifndef RT_PAIR_SKY_CELL
#define RT_PAIR_SKY_CELL 1
#endif
constexpr bool lean_sky_cell(bool pair) { return pair && RT_PAIR_SKY_CELL != 0; }

#if defined(__HIP_DEVICE_COMPILE__)
// ---- device: hipcc's f32 division and square root without the identity steps (see the header comment) ----

// r1 of the expansion: v_rcp_f32 and one Newton step.  d tame.
__device__ __forceinline__ float lean_rcp_refined(float d)
{
	const float r0 = __builtin_amdgcn_rcpf(d);
	const float e = __builtin_fmaf(-d, r0, 1.0f);
	return __builtin_fmaf(e, r0, r0);
}
// quotient from the refined reciprocal: mul, then two (residual, correction) pairs; the last fma is v_div_fmas with VCC = 0
__device__ __forceinline__ float lean_div_core(float n, float d, float r1)
{
	const float q0 = n * r1;
	const float e1 = __builtin_fmaf(-d, q0, n);
	const float q1 = __builtin_fmaf(e1, r1, q0);
	const float e2 = __builtin_fmaf(-d, q1, n);
	return __builtin_fmaf(e2, r1, q1);
}
// n / d, both tame (|n|, |d| in [2^-81, 2^41], exponent difference < 96)
__device__ __forceinline__ float lean_div(float n, float d) { return lean_div_core(n, d, lean_rcp_refined(d)); }
// n / d, d tame, n tame OR zero / infinite / NaN (v_div_fixup_f32 supplies the IEEE result for those, as in `n / d`)
__device__ __forceinline__ float lean_div_fix(float n, float d)
{
	return __builtin_amdgcn_div_fixupf(lean_div_core(n, d, lean_rcp_refined(d)), d, n);
}
// 1 / d, d tame: q0 = 1 * r1 is r1 itself
__device__ __forceinline__ float lean_inv(float d)
{
	const float r1 = lean_rcp_refined(d);
	const float e1 = __builtin_fmaf(-d, r1, 1.0f);
	const float q1 = __builtin_fmaf(e1, r1, r1);
	const float e2 = __builtin_fmaf(-d, q1, 1.0f);
	return __builtin_fmaf(e2, r1, q1);
}
// 1 / d, d tame, ON GFX950: the refined reciprocal IS the quotient.  hipcc's expansion (lean_inv) must hold for any v_rcp_f32
// within 1 ulp and therefore corrects r1 twice; gfx950's v_rcp_f32 is one fixed function, and 1 / d is scale-invariant while
// nothing leaves the normal range, so the 2^23 significands decide whether a correction ever changes a bit.  None does:
// rt_selftest_short_forms (rt_selftest_forms.hip) runs r1, r1 with one correction pair and lean_inv against `1.0f / d` ON THE
// DEVICE over every significand, both signs, at the exponents -81, -60, -24, -1, 0, 1, 24 and 41 (the ends of the tame range and
// between) -- 134 217 728 inputs, no mismatch for any of the three (profiles/r07_short_forms_enumeration.txt);
// tests/test_gpu_short_forms.py asserts it on every build.  Three instructions instead of seven.  A statement about gfx950 only.
__device__ __forceinline__ float lean_inv_gfx950(float d) { return lean_rcp_refined(d); }
// the one lean_inv_form names for the feature set
template <bool PAIR> __device__ __forceinline__ float lean_inv_for(float d)
{
	return lean_inv_form(PAIR) == LeanInvForm::refined ? lean_inv_gfx950(d) : lean_inv(d);
}
// v / d componentwise with ONE refined reciprocal; v's components and d tame
__device__ __forceinline__ V3 lean_div3(V3 v, float d)
{
	const float r1 = lean_rcp_refined(d);
	return V3{lean_div_core(v.x, d, r1), lean_div_core(v.y, d, r1), lean_div_core(v.z, d, r1)};
}
// ... components tame or zero / infinite / NaN
__device__ __forceinline__ V3 lean_div3_fix(V3 v, float d)
{
	const float r1 = lean_rcp_refined(d);
	return V3{__builtin_amdgcn_div_fixupf(lean_div_core(v.x, d, r1), d, v.x), __builtin_amdgcn_div_fixupf(lean_div_core(v.y, d, r1), d, v.y),
	          __builtin_amdgcn_div_fixupf(lean_div_core(v.z, d, r1), d, v.z)};
}

// n / d, both tame, ON GFX950: the quotient from the refined reciprocal with ONE (residual, correction) pair.  hipcc's expansion
// (lean_div_core) corrects twice because its r1 is only known to be close; on gfx950 r1 IS RN(1 / d) for every tame d
// (lean_inv_gfx950 above), and with a correctly rounded reciprocal q0 = n * r1, e = fma(-d, q0, n), q = fma(e, r1, q0) is the
// classical one-step correction.  Theory leaves denominators with an all-ones significand open, so the claim rests on enumeration:
// rt_selftest_div_forms (rt_selftest_forms.hip) runs this form, lean_div_core and `n / d` side by side ON THE DEVICE; n / d is
// scale-invariant while nothing leaves the normal range, so all 2^23 x 2^23 significand pairs at exponents (0, 0) decide it, and
// the ends of the tame range are run for the denominators most likely to differ (profiles/r09_div_forms_enumeration.txt: no
// mismatch); tests/test_gpu_div_forms.py asserts a slice of it on every build.  Six instructions instead of eight, and four
// instead of six per further quotient by the same d.  A statement about gfx950 only.
__device__ __forceinline__ float lean_div_core_gfx950(float n, float d, float r1)
{
	const float q0 = n * r1;
	const float e = __builtin_fmaf(-d, q0, n);
	return __builtin_fmaf(e, r1, q0);
}
// the core lean_div_form names for the feature set
template <bool PAIR> __device__ __forceinline__ float lean_div_core_for(float n, float d, float r1)
{
	return lean_div_form(PAIR) == LeanDivForm::one_pair ? lean_div_core_gfx950(n, d, r1) : lean_div_core(n, d, r1);
}
// lean_div, lean_div_fix and lean_div3_fix (same domains) over that core
template <bool PAIR> __device__ __forceinline__ float lean_div_for(float n, float d) { return lean_div_core_for<PAIR>(n, d, lean_rcp_refined(d)); }
template <bool PAIR> __device__ __forceinline__ float lean_div_fix_for(float n, float d)
{
	return __builtin_amdgcn_div_fixupf(lean_div_core_for<PAIR>(n, d, lean_rcp_refined(d)), d, n);
}
template <bool PAIR> __device__ __forceinline__ V3 lean_div3_for(V3 v, float d)
{
	const float r1 = lean_rcp_refined(d);
	return V3{lean_div_core_for<PAIR>(v.x, d, r1), lean_div_core_for<PAIR>(v.y, d, r1), lean_div_core_for<PAIR>(v.z, d, r1)};
}
template <bool PAIR> __device__ __forceinline__ V3 lean_div3_fix_for(V3 v, float d)
{
	const float r1 = lean_rcp_refined(d);
	return V3{__builtin_amdgcn_div_fixupf(lean_div_core_for<PAIR>(v.x, d, r1), d, v.x), __builtin_amdgcn_div_fixupf(lean_div_core_for<PAIR>(v.y, d, r1), d, v.y),
	          __builtin_amdgcn_div_fixupf(lean_div_core_for<PAIR>(v.z, d, r1), d, v.z)};
}

// sqrtf(x) for x in {+-0} U [2^-96, +inf] U NaN U [-inf, -2^-126]: v_sqrt_f32 (1 ulp) and the expansion's two one-ulp corrections.
// NOT the negative denormals: v_sqrt_f32 takes them for -0 and returns -0 where sqrtf returns NaN (all 2^23 - 1 of them differ).
// Both corrections are needed on gfx950: over every float of this domain v_sqrt_f32 is one ulp low 283 860 640 times and one ulp
// high 109 984 times (rt_selftest_short_forms), so neither can be dropped.
// The 2^32 pre-scale the expansion applies below 2^-96 and its final class test (which returns x itself for +-0 and +inf)
// are the identity there: for x = +-0 both corrections compare NaN / +-0 residuals and keep v_sqrt's +-0, for +inf they keep inf.
__device__ __forceinline__ float lean_sqrt(float x)
{
	const float s = __builtin_amdgcn_sqrtf(x);
	const float s_dn = __uint_as_float(__float_as_uint(s) - 1u);
	const float s_up = __uint_as_float(__float_as_uint(s) + 1u);
	const float r_dn = __builtin_fmaf(-s_dn, s, x);
	const float r_up = __builtin_fmaf(-s_up, s, x);
	float r = (r_dn <= 0.0f) ? s_dn : s;
	r = (r_up > 0.0f) ? s_up : r;
	return r;
}
// smallest input the short form is exact for
constexpr float kLeanSqrtMin = 0x1p-96f;

// the divisions inside rt_atan2f on the device: the octant fold (t - 1) / (t + 1) has t in [0, 1] (NaN when 0 / 0 or
// inf / inf, where the result is overridden): numerator zero or of magnitude >= 2^-24, denominator in [1, 2]
__device__ __forceinline__ float lean_atan2(float y, float x)
{
	return lean_atan2_with(y, x, [](float n, float d) { return n / d; }, [](float n, float d) { return lean_div_fix(n, d); });
}
// ... with the octant fold through the form lean_div_form names (same operands, same domain).  The ratio min / max stays on the
// plain operator: its operands are whatever the caller's vector holds, and the test that would admit them costs what the short
// form saves.  PAIR = false is lean_atan2.
template <bool PAIR> __device__ __forceinline__ float lean_atan2_for(float y, float x)
{
	return lean_atan2_with(y, x, [](float n, float d) { return n / d; }, [](float n, float d) { return lean_div_fix_for<PAIR>(n, d); });
}
// acos with the short square root: 0.5 * (1 - |x|) is zero, negative, NaN or >= 2^-25
__device__ __forceinline__ float lean_acos_dev(float x) { return lean_acos_with(x, lean_sqrt(0.5f * (1.0f - fabsf(x)))); }
#else
// host pass of the same translation units (kernel bodies are parsed, never run, there): the plain operators
RT_FN float lean_rcp_refined(float d) { return 1.0f / d; }
RT_FN float lean_div_core(float n, float d, float) { return n / d; }
RT_FN float lean_div(float n, float d) { return n / d; }
RT_FN float lean_div_fix(float n, float d) { return n / d; }
RT_FN float lean_inv(float d) { return 1.0f / d; }
RT_FN V3 lean_div3(V3 v, float d) { return v / d; }
RT_FN V3 lean_div3_fix(V3 v, float d) { return v / d; }
RT_FN float lean_sqrt(float x) { return sqrtf(x); }
constexpr float kLeanSqrtMin = 0x1p-96f;
RT_FN float lean_inv_gfx950(float d) { return 1.0f / d; }
template <bool PAIR> RT_FN float lean_inv_for(float d) { return 1.0f / d; }
RT_FN float lean_div_core_gfx950(float n, float d, float) { return n / d; }
template <bool PAIR> RT_FN float lean_div_core_for(float n, float d, float) { return n / d; }
template <bool PAIR> RT_FN float lean_div_for(float n, float d) { return n / d; }
template <bool PAIR> RT_FN float lean_div_fix_for(float n, float d) { return n / d; }
template <bool PAIR> RT_FN V3 lean_div3_for(V3 v, float d) { return v / d; }
template <bool PAIR> RT_FN V3 lean_div3_fix_for(V3 v, float d) { return v / d; }
template <bool PAIR> RT_FN float lean_atan2_for(float y, float x) { return lean_atan2_portable(y, x); }
RT_FN float lean_atan2(float y, float x) { return lean_atan2_portable(y, x); }
RT_FN float lean_acos_dev(float x) { return lean_acos(x); }
#endif

} // namespace rt
