// pair_shadow_check.cpp -- the two-sphere kernels' occlusion predicate for a ray without a limit (raytracing-rust_amd/csrc/
// rt_intersect.h sphere_occludes_unlimited, and the branch-free full test behind it, sphere_occludes_asked) against Sphere::get_int's
// `hit && t > 0` (sphere_t), on the host: its `/` and sqrtf are the arithmetic contract's operators.  Built by
// tests/test_pair_shadow_host.py with `hipcc --cuda-host-only -fsanitize=address,undefined`.
// With a file name as its argument it runs the edge grid alone and writes the grid's cases there, 10 floats each (centre, radius,
// origin, direction), for the device self-test to run the same operands (tests/test_gpu_pair_shadow.py).
// Prints one line per operand set: "<name> <cases> <mismatches> <mismatches of the full test's form> <cases the signs could not settle>".
#include <cmath>
#include <limits>
#include "../../raytracing-rust_amd/csrc/rt_intersect.h"
#include "check_common.h"

using rt::Ray;
using rt::V3;

struct Tally {
	unsigned long long n = 0, bad = 0, bad_asked = 0, asked = 0;
	std::vector<float> *keep = nullptr; // the cases as run, when they are to be written out
	void run(V3 center, float radius, V3 origin, V3 direction)
	{
		if (keep)
			keep->insert(keep->end(), {center.x, center.y, center.z, radius, origin.x, origin.y, origin.z, direction.x, direction.y, direction.z});
		Ray r;
		r.o = origin;
		r.d = direction;
		r.inv = r.shear = rt::v3s(0.0f); // (no sphere test reads them)
		float t = 0.0f;
		const bool want = rt::sphere_t(center, radius, r, t) && t > 0.0f;
		bad += rt::sphere_occludes_unlimited(center, radius, r) != want;
		bad_asked += rt::sphere_occludes_asked(center, radius, r) != want;
		asked += rt::sphere_shadow_signs(center, radius, r).ask;
		++n;
	}
	void print(const char *name) const { std::printf("%s %llu %llu %llu %llu\n", name, n, bad, bad_asked, asked); }
};

int main(int argc, char **argv)
{
	const bool grid_only = argc > 1;
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const float denorm = f_of(1u), denorm_big = f_of(0x007FFFFFu);

	// ---- seeded random rays and spheres: the shapes a render produces (unit directions, origins on and around the spheres, radii
	// over twelve decades), a share of them with the origin ON the surface as a shadow ray's is
	Tally rnd;
	for (int i = 0; i < (grid_only ? 0 : 10000000); ++i) {
		const float radius = std::exp2f(40.0f * unit() - 20.0f);
		const V3 center = rt::v3(4.0f * signed_unit(), 4.0f * signed_unit(), 4.0f * signed_unit());
		V3 n = rt::v3(signed_unit(), signed_unit(), signed_unit());
		n = n / rt::mag(n);
		V3 d = rt::v3(signed_unit(), signed_unit(), signed_unit());
		d = d / rt::mag(d);
		const uint32_t where = next_u32() & 7u; // 0-2 on the surface (offset as do_light offsets it), 3 inside, 4 near outside, 5-7 far
		float dist = 1.0f;
		if (where <= 2u)
			dist = 1.0f + (where == 0u ? 0.0f : where == 1u ? 1e-4f : -1e-4f) / radius;
		else if (where == 3u)
			dist = unit();
		else if (where == 4u)
			dist = 1.0f + unit();
		else
			dist = 1.0f + std::exp2f(20.0f * unit());
		rnd.run(center, radius, center + (radius * dist) * n, d);
	}
	if (!grid_only)
		rnd.print("random");

	// ---- the edge grid: every combination of a radius, an origin placement and a direction from the lists below
	Tally grid;
	std::vector<float> cases;
	if (grid_only)
		grid.keep = &cases;
	const float radii[] = {0x1p-70f, 1.0f, 0x1p58f, 0x1p59f, 0x1p59f * (1.0f + 0x1p-23f), 0x1p60f, 0x1p100f, inf, denorm, -1.0f, nan};
	// the origin as centre - deltap along x, with |deltap|^2 - radius^2 = c landing on 0, +-denormals, +-2^-61, +-2^-60 where the
	// radius allows it (radius 1: deltap^2 = 1 + c is not representable for the tiny c, so the offsets below are applied to deltap
	// directly, and again with a tiny radius where c IS the tiny number), and on plainly inside / outside
	const float scale[] = {0.0f, 0.5f, 1.0f - 0x1p-24f, 1.0f, 1.0f + 0x1p-23f, 2.0f, 0x1p30f};
	const float tiny[] = {0.0f, -0.0f, denorm, -denorm, denorm_big, 0x1p-61f, 0x1p-60f, 0x1.6a09e6p-31f, 0x1p-30f, 0x1p-31f};
	const V3 dirs[] = {{1, 0, 0},   {-1, 0, 0},       {0, 1, 0},      {0, 0, -1},        {0, 0, 0},         {0.6f, 0.8f, 0},   {-0.6f, 0, 0.8f},
	                   {inf, 0, 0}, {-inf, 0, 0},     {nan, 0, 0},    {0, nan, 1},       {0x1p100f, 0, 0},  {-0x1p100f, 1, 0}, {0x1p-100f, 0, 0},
	                   {-0.0f, 0, 0}, {1, 1, 1},      {-1, -1, -1},   {denorm, 0, 0},    {-denorm, 0, 0},   {0x1p60f, 0, 0},   {-0x1p60f, 0, 0},
	                   {0x1p59f, 0, 0}, {-0x1p59f, 0, 0}, {-0x1p59f * (1.0f + 0x1p-23f), 0, 0}};
	for (float radius : radii)
		for (const V3 &d : dirs) {
			for (float s : scale)
				for (int axis = 0; axis < 3; ++axis) {
					const float off = radius * s;
					grid.run(rt::v3(1.0f, -2.0f, 0.5f), radius, rt::v3(1.0f, -2.0f, 0.5f) - rt::v3(axis == 0 ? off : 0.0f, axis == 1 ? off : 0.0f, axis == 2 ? off : 0.0f), d);
					grid.run(rt::v3s(0.0f), radius, rt::v3(axis == 0 ? -off : 0.0f, axis == 1 ? off : 0.0f, axis == 2 ? -off : 0.0f), d);
				}
			// deltap itself tiny (c = deltap^2 - radius^2 lands on +-0, denormals, +-2^-61, +-2^-60 with radius 2^-70 or a denormal),
			// and radius^2 + tiny with radius 2^-31 .. 2^-30
			for (float a : tiny)
				for (float b : tiny) {
					grid.run(rt::v3s(0.0f), radius, rt::v3(a, b, 0.0f), d);
					grid.run(rt::v3s(0.0f), a, rt::v3(b, 0.0f, 0.0f), d);
					grid.run(rt::v3s(0.0f), a, rt::v3(0.0f, -b, a), d);
				}
		}
	// discriminant at 0, denormal and inf: a tangent ray, a ray whose remedy term squares to radius^2 minus a denormal, a huge radius
	const V3 yhat = rt::v3(0, 1, 0);
	const float offs[] = {1.0f, 1.0f - 0x1p-24f, 1.0f + 0x1p-23f, 0x1p-64f, 0x1p-64f * (1.0f - 0x1p-24f), 0x1p-75f, 0x1p-74f};
	for (float rad : {1.0f, 0x1p-64f, 0x1p-75f, 0x1p64f, 0x1p127f})
		for (float o : offs)
			for (float back : {-2.0f, 0.0f, -0.0f, 2.0f, 0x1p-70f, -0x1p-70f}) {
				grid.run(rt::v3s(0.0f), rad, rt::v3(o, back, 0.0f), yhat);
				grid.run(rt::v3s(0.0f), rad, rt::v3(o * rad, back * rad, 0.0f), yhat);
				grid.run(rt::v3s(0.0f), rad, rt::v3(o, back, 0.0f), -yhat);
			}
	grid.print("grid");
	return grid_only ? write_cases(argv[1], cases) : 0;
}
