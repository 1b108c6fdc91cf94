// rt_sky_cell.h -- the host's side of the carried sky cell (rt_shade.h sky_sample_cell / sky_pdf_carried; the proof stands there):
// per scene, the bounds E_u, E_v of that proof evaluated in double and rounded outward, the jitter margins delta = 2 E they license,
// and the row range.  HIP-free and header-only: rt_api.cpp fills the scene's DevSkyCell (rt_types.h; RenderArgs::sky_cell) from it, tests/cpp/sky_cell_check.cpp runs it against a
// brute-force round trip in double.
#pragma once
#include <cmath>
#include <cstdint>

namespace rt {

struct SkyCellGuard {
	uint32_t ok;              // 0: the kernels keep sky_pdf's own round trip for every lane
	float half_u, half_v;     // 0.5 - delta of each axis: a jitter r is guarded when |r - 0.5| <= half (exact for r, delta multiples of 2^-24)
	uint32_t row_lo, row_span; // rows row_lo .. row_lo + row_span are guarded
	double e_u, e_v;          // the proof's bounds, in cells
	double delta_u, delta_v;  // 2 E rounded up to a multiple of 2^-24
	double s_edge;            // smallest sine over the edges of the guarded rows, rounded down
};

constexpr double kSkyCellSafety = 2.0;   // every stated ulp figure of rt_detmath.h may double (rt_shade.h)
constexpr double kSkyCellOutward = 1.0 + 0x1p-30; // libm's sin, the sums and products below: far inside
constexpr uint32_t kSkyCellMaxRes = 1u << 15;     // su | sv << 16 | ok << 31 is one word

// `reciprocals_verified`: DevSky::inv_res_ok of the same scene (rt_api.cpp sky_reciprocals)
inline SkyCellGuard sky_cell_guard(uint32_t rx, uint32_t ry, bool reciprocals_verified)
{
	SkyCellGuard g = {};
	if (!reciprocals_verified || rx == 0u || ry < 3u || rx >= kSkyCellMaxRes || ry >= kSkyCellMaxRes)
		return g;
	const double e = 0x1p-24, pi = 3.14159265358979323846, k_pi = (double)3.14159274101257324219f;
	const uint32_t row_lo = 1u, row_hi = ry - 2u;
	// the guarded rows' outer edges, as the angles the kernels' kPi puts them at: row_lo kPi / ry and (row_hi + 1) kPi / ry
	const double s_lo = std::sin(k_pi * row_lo / ry), s_hi = std::sin(pi - k_pi * (row_hi + 1u) / ry);
	const double s_edge = std::fmin(s_lo, s_hi) / kSkyCellOutward;
	if (!(s_edge >= 0x1p-8))
		return g;
	const double e_v = ((double)ry * (12.0 * e) + ((double)ry / pi) * (4.0 * e + 0x1p-45) / s_edge) * kSkyCellOutward;
	const double e_u = ((double)rx * (7.0 * e) + ((double)rx / (2.0 * pi)) * (40.0 * e + 0x1p-44)) * kSkyCellOutward;
	const double d_u = std::ceil(kSkyCellSafety * e_u * 0x1p24) * e, d_v = std::ceil(kSkyCellSafety * e_v * 0x1p24) * e;
	g.e_u = e_u;
	g.e_v = e_v;
	g.delta_u = d_u;
	g.delta_v = d_v;
	g.s_edge = s_edge;
	if (!(d_u < 0.25 && d_v < 0.25))
		return g;
	g.half_u = (float)(0.5 - d_u); // exact: multiples of 2^-24 in (0.25, 0.5]
	g.half_v = (float)(0.5 - d_v);
	g.row_lo = row_lo;
	g.row_span = row_hi - row_lo;
	g.ok = 1u;
	return g;
}

} // namespace rt
