// rt_selftest_dev.h -- device helpers the self-test translation units share (rt_selftest.hip, rt_selftest_forms.hip).
#pragma once

#include "rt_intersect.h"

namespace rt {

__device__ __forceinline__ bool same_f32(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
__device__ __noinline__ Ray ray_new_plain(V3 origin, V3 direction) // the plain operators, kept out of line so nothing is shared with the short form
{
	Ray r;
	direction = direction / mag(direction);
	r.o = origin;
	r.d = direction;
	r.inv = v3(1.0f / direction.x, 1.0f / direction.y, 1.0f / direction.z);
	const float ax = fabsf(direction.x), ay = fabsf(direction.y), az = fabsf(direction.z);
	const bool swap = (ax > ay && ax > az) || (ay > az);
	const float sx = swap ? direction.z : direction.x;
	const float sz = swap ? direction.x : direction.z;
	r.shear = v3(-sx / sz, -direction.y / sz, 1.0f / sz);
	return r;
}

} // namespace rt
