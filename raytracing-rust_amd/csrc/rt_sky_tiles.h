// rt_sky_tiles.h -- FeatPair: a per-pixel proof that no primary ray of the pixel can hit either sphere (host + device), the block
// of launch constants it reads (host, double precision) and the tile rule built on it.  rt_render.hip's acquire_coarse asks it once
// per claim and runs flagged tiles through the sky run; rt_selftest_sky_tiles runs the same inline code on the device,
// tests/cpp/sky_tiles_check.cpp on the CPU.
//
// THE TEST.  Every primary ray leaves cam.origin (do_gen never moves it) with a direction from the pixel's footprint
//   g(x, y) = cam_ll + cam_h * (x / (W-1)) + cam_v * (1 - y / (H-1)) - cam_o,   x in [px, px+1], y in [py, py+1]
// (closed: jitter + px may round up to px + 1).  Per sphere s the host supplies a unit vector n_s from the origin to the centre and a
// threshold K_s; the pixel passes when cos(angle(c, n_s)) < K_s for both spheres, c = g(px + 1/2, py + 1/2) formed from
// DevSkyTiles::base / step_x / step_y.  K_s = cos(a_s) - e_cos, rounded down, with
//   a_s = phi0_s + rho + slop,   phi0_s = theta_s + 2 rho (kSkyMarginRho),
//   theta_s = asin(r_s / D_s): the sphere's angular radius (D_s = |deltap_s|, the FLOAT centre - origin the walks use, in double),
//   rho = asin(half_diag / dist): no footprint corner is further than that from its pixel's centre direction -- half_diag =
//         (|cam_h| / (W-1) + |cam_v| / (H-1)) / 2 bounds |g(corner) - g(centre)|, dist = the origin's distance from the image plane
//         bounds |g| from below, and sin(angle(a, b)) <= |a - b| / |a|.  2 rho, one whole pixel diagonal, is the margin,
//   slop = 16 u (1 + M / dist), u = 2^-24, M = |cam_ll| + |cam_h| + |cam_v| + |cam_o|: what do_gen's float arithmetic (u and v to
//         two roundings each, four vector operations: at most 8 u M off in the plane) and ray_new's normalisation (a common scale
//         plus one rounding per component: 2 u) can turn a footprint direction by,
//   e_cos = 16 u (1 + M' / dist), M' = |base| + W |step_x| + H |step_y|: the error of the tested cosine -- c to three roundings per
//         component of inputs rounded once (4 u M' / |c| as an angle), the dot product (3 u), n_s rounded to float (2 u), the
//         square root and the product K * |c| (3 u).
// So a pixel that passes has its exact centre direction more than a_s from n_s, every exact footprint direction more than
// phi0_s + slop, and every direction d ray_new can return for it at an angle phi > phi0_s from n_s.
//
// WHAT FOLLOWS for sphere_t_tail's floats (rt_intersect.h; deltap, c = deltap.deltap - r^2 as sphere_t or DevPairPrimary form them):
//  (A) phi in (phi0, pi - phi0], phi0 < pi/2: the discriminant is not > 0.  d = (1 + e1) d^ with |e1| <= 4 u, so exactly
//      |deltap - (d.deltap) d|^2 = D^2 sin^2(phi) + (d^.deltap)^2 (2 e1 + e1^2)^2 >= D^2 sin^2(phi).  In floats ddp is off by at most
//      3 u D, each component of the remedy term by one rounding of the product and one of the difference: the vector by at most
//      6 u D.  Its squared length is computed to (1 - 3 u): fl(dot) >= (D sin(phi) - 6 u D)^2 (1 - 3 u), and fl(r^2) <= r^2 (1 + u).
//      The float difference of two floats is positive only if the first is larger, so `discriminant > 0` needs
//      r sqrt(1 + u) > (D sin(phi) - 6 u D) sqrt(1 - 3 u), which sin(phi) - sin(theta) >= 16 u rules out.  On the interval
//      sin(phi) >= sin(phi0), and the host verifies sin(phi0) - sin(theta) >= 16 u (else nothing passes).
//  (B) phi > pi - phi0 (phi0 < pi/2), or any phi > phi0 when phi0 >= pi/2: cos(phi) <= -1e-6, so ddp = fl(d.deltap) <= D (cos(phi)
//      (1 - 4 u) + 3 u) < 0, and the host verifies c > 0 in the float the kernel reads.  If the discriminant is > 0, sqrt_val is in
//      (0, inf], q = ddp - sqrt_val < 0, t0 = q < 0 and t1 = c / q <= -0: whichever order the swap leaves them in, `t0 > 0` fails and
//      `t1 <= 0` holds: no hit.  (The line meets the sphere BEHIND the origin; this is why the statement is "no hit", not
//      "no positive discriminant".)
//  A phi0 within 1e-6 of pi/2 is moved to pi/2 + 1e-6, so that one of the two cases always applies.
// Either way sphere_t_tail returns false for both spheres and the walk reports no hit, whatever its box tests say: they only
// decide WHETHER a sphere is tested.  D and r are required in [2^-40, 2^40] (no square over- or underflows), the origin outside
// both spheres; a non-finite camera, a degenerate viewport, W or H below 2 or a scene that is not two spheres gives enabled = 0.
#pragma once

#include <cmath>

#include "rt_types.h"

namespace rt {

#ifndef RT_SKY_MARGIN_RHO
#define RT_SKY_MARGIN_RHO 2.0
#endif
constexpr double kSkyMarginRho = RT_SKY_MARGIN_RHO; // the margin, in pixel half-diagonals (rho)

struct alignas(64) DevSkyTiles {
	float base[3];    // g(1/2, 1/2)
	float step_x[3];  // cam_h / (W-1)
	float step_y[3];  // -cam_v / (H-1)
	float n[2][3];    // [sphere]: unit vector origin -> centre
	float k[2];       // [sphere]: threshold (-2: nothing passes)
	uint32_t enabled; // 0: no tile is ever flagged
	uint32_t pad[14];
};
static_assert(sizeof(DevSkyTiles) == 128, "DevSkyTiles: two 64-byte lines");

// pixel (px, py) passes: the code every side runs (px, py < 65536: exact as floats)
RT_FN bool sky_pixel_passes(const DevSkyTiles &t, uint32_t px, uint32_t py)
{
	const float fx = (float)px, fy = (float)py;
	const V3 c = v3(t.base[0] + t.step_x[0] * fx + t.step_y[0] * fy, t.base[1] + t.step_x[1] * fx + t.step_y[1] * fy,
	                t.base[2] + t.step_x[2] * fx + t.step_y[2] * fy);
	const float len = sqrtf(dot(c, c));
	const bool p0 = dot(c, v3(t.n[0][0], t.n[0][1], t.n[0][2])) < t.k[0] * len;
	const bool p1 = dot(c, v3(t.n[1][0], t.n[1][1], t.n[1][2])) < t.k[1] * len;
	return p0 && p1; // (a NaN anywhere fails)
}
// THE TILE RULE.  A tile of 64 pixels (1 << log2_w wide, origin (x0, y0)) is flagged when every pixel inside the image of the tile
// ITSELF AND OF ITS EIGHT NEIGHBOURS passes: a tile with a pixel that may see a sphere keeps the whole ring of tiles around it in the
// ordinary loop.  The proof above needs the tile's own 64 pixels only; the ring is a margin of one tile on top of the pixel's, so
// that a sphere of any size, however small, clears its own tile and all eight around it.  Lane i of a wave answers for pixel i
// of each of the nine tiles (what acquire_coarse and rt_selftest_sky_tiles run: one ballot of the answers decides the tile);
// pixels outside the image pass.
RT_FN bool sky_lane_passes(const DevSkyTiles &t, uint32_t x0, uint32_t y0, uint32_t log2_w, uint32_t lane, uint32_t width, uint32_t height)
{
	const int32_t tw = (int32_t)(1u << log2_w), th = (int32_t)(64u >> log2_w);
	const int32_t lx = (int32_t)x0 + (int32_t)(lane & ((1u << log2_w) - 1u)), ly = (int32_t)y0 + (int32_t)(lane >> log2_w);
	bool ok = true;
	for (int32_t b = -1; b <= 1; ++b)
		for (int32_t a = -1; a <= 1; ++a) {
			const int32_t px = lx + a * tw, py = ly + b * th;
			const bool outside = px < 0 || py < 0 || px >= (int32_t)width || py >= (int32_t)height;
			ok = ok && (outside || sky_pixel_passes(t, (uint32_t)px, (uint32_t)py));
		}
	return ok;
}
inline bool sky_tile_passes(const DevSkyTiles &t, uint32_t x0, uint32_t y0, uint32_t log2_w, uint32_t width, uint32_t height)
{
	if (t.enabled == 0u)
		return false;
	for (uint32_t lane = 0; lane < 64u; ++lane)
		if (!sky_lane_passes(t, x0, y0, log2_w, lane, width, height))
			return false;
	return true;
}

// the block for this scene, camera and image size (host; double precision, thresholds rounded towards "fewer tiles pass")
inline void sky_tiles_terms(const DevPairScene &q, const DevPairPrimary &pp, const DevCamera &cam, uint32_t width, uint32_t height, DevSkyTiles &t)
{
	t = DevSkyTiles{};
	t.k[0] = t.k[1] = -2.0f;
	if (width < 2u || height < 2u || width >= 65536u || height >= 65536u || pp.valid == 0u)
		return;
	const double u = 0x1p-24, pi = 3.14159265358979323846;
	double o[3], ll[3], h[3], v[3], base[3], sx[3], sy[3];
	for (int i = 0; i < 3; ++i) {
		o[i] = cam.origin[i]; ll[i] = cam.lower_left[i]; h[i] = cam.horizontal[i]; v[i] = cam.vertical[i];
		if (!std::isfinite(o[i]) || !std::isfinite(ll[i]) || !std::isfinite(h[i]) || !std::isfinite(v[i]))
			return;
		sx[i] = h[i] / (double)(width - 1u);
		sy[i] = -v[i] / (double)(height - 1u);
		base[i] = ll[i] - o[i] + h[i] * (0.5 / (double)(width - 1u)) + v[i] * (1.0 - 0.5 / (double)(height - 1u));
	}
	auto norm = [](const double a[3]) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
	// the origin's distance from the image plane, in which every g lies
	const double nrm[3] = {h[1] * v[2] - h[2] * v[1], h[2] * v[0] - h[0] * v[2], h[0] * v[1] - h[1] * v[0]};
	const double g0[3] = {ll[0] - o[0], ll[1] - o[1], ll[2] - o[2]};
	const double nn = norm(nrm);
	if (!(nn > 0.0) || !std::isfinite(nn))
		return;
	const double dist = std::fabs(g0[0] * nrm[0] + g0[1] * nrm[1] + g0[2] * nrm[2]) / nn;
	const double M = norm(ll) + norm(h) + norm(v) + norm(o);
	const double Mc = norm(base) + (double)width * norm(sx) + (double)height * norm(sy);
	const double half_diag = 0.5 * (norm(h) / (double)(width - 1u) + norm(v) / (double)(height - 1u));
	if (!(dist > 0.0) || !std::isfinite(dist) || !std::isfinite(M) || !std::isfinite(Mc) || !(half_diag < dist))
		return;
	const double rho = std::asin(half_diag / dist);
	const double slop = 16.0 * u * (1.0 + M / dist), e_cos = 16.0 * u * (1.0 + Mc / dist);
	if (!(slop < 1e-3) || !(e_cos < 1e-3))
		return;
	for (int i = 0; i < 3; ++i) {
		t.base[i] = (float)base[i]; t.step_x[i] = (float)sx[i]; t.step_y[i] = (float)sy[i];
		if (!std::isfinite(t.base[i]) || !std::isfinite(t.step_x[i]) || !std::isfinite(t.step_y[i]))
			return;
	}
	for (int s = 0; s < 2; ++s) {
		const double dp[3] = {pp.sphere[s][0], pp.sphere[s][1], pp.sphere[s][2]}; // the float deltap of the walks
		const double D = norm(dp), r = std::fabs((double)q.sphere[s][3]);
		for (int i = 0; i < 3; ++i)
			t.n[s][i] = D > 0.0 ? (float)(dp[i] / D) : 0.0f;
		if (!(pp.sphere[s][3] > 0.0f) || !(r < D) || !(D >= 0x1p-40 && D <= 0x1p40) || !(r >= 0x1p-40 && r <= 0x1p40))
			continue; // the origin inside or on the sphere, or sizes the error model does not cover: nothing passes
		const double theta = std::asin(r / D);
		double phi0 = theta + kSkyMarginRho * rho;
		if (phi0 > pi / 2 - 1e-6)
			phi0 = std::fmax(phi0, pi / 2 + 1e-6); // case (B) alone
		else if (!(std::sin(phi0) - std::sin(theta) >= 16.0 * u))
			continue;
		const double a = phi0 + rho + slop;
		if (!(a < pi))
			continue;
		float k = (float)(std::cos(a) - e_cos);
		k = std::nextafterf(std::nextafterf(k, -3.0f), -3.0f); // down past the conversion's own rounding
		t.k[s] = k;
	}
	t.enabled = 1u;
}

} // namespace rt
