// frame_forms_check.cpp -- the scatter frame as the two-sphere kernels form it (raytracing-rust_amd/csrc/rt_shade.h
// coord_from_z_pair: the arm chosen once by selects on the operands, one guard, a literal zero component on the lanes that pass)
// against the two-arm coord_from_z, bit for bit, on the host.  Here the short forms are the plain operators, so what this checks is
// the ALGEBRA of the rewrite: arm choice, operand signs, the zero component and every class of input that fails the guard.  What
// gfx950's instructions return is compared on the device (tests/test_gpu_frame_forms.py).  Built by tests/test_frame_forms_host.py
// with `hipcc --cuda-host-only -ffp-contract=off -fsanitize=address,undefined`.
// With a file name as its argument it runs the edge grid alone and writes the grid's vectors there, 3 floats each, for the device
// self-test to run the same operands.
// Prints one line per operand set: "<name> <vectors> <frames that differ> <vectors that pass the guard> <vectors that fail it>".
#include <cmath>
#include <limits>
#include "../../raytracing-rust_amd/csrc/rt_shade.h"
#include "check_common.h"

using rt::Coord;
using rt::V3;

struct Tally {
	unsigned long long n = 0, bad = 0, pass = 0;
	std::vector<float> *keep = nullptr; // the vectors as run, when they are to be written out
	void run(V3 z)
	{
		if (keep)
			keep->insert(keep->end(), {z.x, z.y, z.z});
		const Coord got = rt::coord_from_z_pair(z), want = rt::coord_from_z(z);
		const bool same = same_v3(got.x, want.x) && same_v3(got.y, want.y) && same_v3(got.z, want.z);
		if (!same && bad < 5)
			std::fprintf(stderr, "differs at (%a, %a, %a)\n", z.x, z.y, z.z);
		bad += !same;
		const float a = std::fabs(z.x) > std::fabs(z.y) ? z.x : z.y;
		pass += rt::frame_guard_(a, z.z, a * a + z.z * z.z);
		++n;
	}
	void print(const char *name) const { std::printf("%s %llu %llu %llu %llu\n", name, n, bad, pass, n - pass); }
};

int main(int argc, char **argv)
{
	const bool grid_only = argc > 1;
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

	// ---- seeded random unit normals, as a sphere's hit record holds them
	Tally rnd;
	for (int i = 0; i < (grid_only ? 0 : 1000000); ++i) {
		V3 n = rt::v3(signed_unit(), signed_unit(), signed_unit());
		n = n / rt::mag(n);
		rnd.run(n);
	}
	if (!grid_only)
		rnd.print("random");

	// ---- the edge grid: every triple of the values below -- axis vectors, |z.x| == |z.y| ties of either sign, +-0 and denormal
	// components, both sides of the guard's bounds (a component at 2^-61 / 2^-60 / 2^-59; s2 around 2^-40 and 2^40 from components
	// at 2^-21 / 2^-20 / 2^-19, 2^19 / 2^20 / 2^21 and at sqrt(1/2) x 2^-20 and x 2^20 with their neighbours), huge, infinite and
	// NaN components in each slot
	const float h = 0.707106769f; // RN(sqrt(1/2)): two such components put s2 next to a power of two, the neighbours on either side of it
	const float values[] = {0.0f, -0.0f, f_of(1u), -f_of(1u), f_of(0x007FFFFFu), 0x1p-61f, 0x1p-60f, -0x1p-60f, 0x1p-59f, f_of(bits_of(0x1p-60f) - 1u),
	                        0x1p-21f, 0x1p-20f, 0x1p-19f, h * 0x1p-20f, f_of(bits_of(h * 0x1p-20f) - 1u), f_of(bits_of(h * 0x1p-20f) + 1u),
	                        1.0f, -1.0f, 0.6f, 0.8f, -h, 0x1p19f, 0x1p20f, -0x1p20f, 0x1p21f, h * 0x1p20f, f_of(bits_of(h * 0x1p20f) - 1u),
	                        f_of(bits_of(h * 0x1p20f) + 1u), 0x1p100f, inf, -inf, nan};
	Tally grid;
	std::vector<float> kept;
	if (grid_only)
		grid.keep = &kept;
	for (float x : values)
		for (float y : values)
			for (float z : values)
				grid.run(rt::v3(x, y, z));
	grid.print("grid");
	return grid_only ? write_cases(argv[1], kept) : 0;
}
