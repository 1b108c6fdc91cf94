// rt_selftest_dev.h -- device helpers the self-test translation units share (rt_selftest.hip, rt_selftest_forms.hip).
#pragma once

#include <algorithm>

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

// ---- what every kernel of rt_selftest_forms.hip is built from: one case loop, one tally, one launcher.  A new self-test writes
// its comparison inside for_each_case and names its counters; nothing below is repeated per form. ----

// body(i) for every i < n, grid-stride: any grid runs every case exactly once
template <class Body> __device__ __forceinline__ void for_each_case(uint64_t n, Body body)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		body(i);
}

// N integer counters a lane keeps while it loops, with the smallest index noted per counter; flush adds each non-zero one to
// counts[k] and, where first indices are kept, lowers first_index[k] -- deterministic whatever the schedule.  Every k is a
// compile-time constant at its call site, so after inlining the counters are registers and the unused ones are gone.
template <int N> struct Tally {
	unsigned long long n[N], first[N];
	__device__ __forceinline__ Tally()
	{
#pragma unroll
		for (int k = 0; k < N; ++k) {
			n[k] = 0ull;
			first[k] = ~0ull;
		}
	}
	__device__ __forceinline__ void add(int k, unsigned long long by = 1ull) { n[k] += by; }
	__device__ __forceinline__ void note(int k, bool differs, unsigned long long index)
	{
		if (differs) {
			n[k] += 1ull;
			first[k] = index < first[k] ? index : first[k];
		}
	}
	__device__ __forceinline__ void flush(unsigned long long *counts, unsigned long long *first_index = nullptr) const
	{
#pragma unroll
		for (int k = 0; k < N; ++k)
			if (n[k]) {
				atomicAdd(&counts[k], n[k]);
				if (first_index)
					atomicMin(&first_index[k], first[k]);
			}
	}
};

// one launch of `kernel` over n_items grid-stride items (n_items >= 1): 256 lanes a block, never more than max_blocks blocks
template <class... Params, class... Args>
inline hipError_t launch_cases(void (*kernel)(Params...), hipStream_t stream, uint64_t n_items, uint32_t max_blocks, const Args &...args)
{
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_items + 255u) / 256u, max_blocks);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, args...);
	return hipGetLastError();
}

} // namespace rt
