// rt_query.hip -- the kernels that answer questions about a scene without rendering it: the batch hit queries
// (rt_check_hit / rt_check_hit_index, include/rt_hip.h) and, in the diagnostic build, the traversal-only trace queue
// (rt_debug_trace_queue).  They walk the trees with the render kernels' own code (rt_intersect.h, rt_shade.h) and share no
// translation unit with them: an edit here rebuilds no render kernel and moves none of their register allocation.
#include "rt_shade.h"
#include "rt_query.h"

namespace rt {

// ---- batch hit queries (AccelerationStructure::check_hit / check_hit_index) ----
struct DevRayDesc {
	float origin[3], direction[3];
};
struct DevHitRecord {
	float t, point[3], error[3], normal[3], uv[2];
	int32_t has_uv, out;
	uint32_t material, found;
	unsigned long long index;
};
static_assert(sizeof(DevHitRecord) == 72, "must match rt_hit_record");

__device__ __forceinline__ void store_record(DevHitRecord &o, const Hit &h, uint32_t material, unsigned long long index, bool found)
{
	o.t = h.t;
	o.point[0] = h.point.x; o.point[1] = h.point.y; o.point[2] = h.point.z;
	o.error[0] = h.error.x; o.error[1] = h.error.y; o.error[2] = h.error.z;
	o.normal[0] = h.normal.x; o.normal[1] = h.normal.y; o.normal[2] = h.normal.z;
	o.uv[0] = h.uvx; o.uv[1] = h.uvy;
	o.has_uv = h.has_uv ? 1 : 0;
	o.out = h.out ? 1 : 0;
	o.material = mat_handle_index(material); // (the caller's index, not the handle the kernels carry)
	o.found = found ? 1u : 0u;
	o.index = index;
}

template <bool PRUNE>
__global__ __launch_bounds__(256) void check_hit_kernel(const DevScene S, const DevRayDesc *__restrict__ rays, uint64_t n,
                                                        DevHitRecord *__restrict__ outr)
{
	using F = FeatFull; // batch queries serve every scene: all primitive types compiled in
	extern __shared__ __align__(16) uint32_t lds[];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t *stk = lds + wave * (S.stack_depth * kStackStride) + lane;
	// the whole worst case in LDS: the overflow branch is never taken (its base only has to be some global pointer;
	// a literal null there sends this compiler's SimplifyCFG into a crash)
	const StackMem SM = {S.stack_depth, 0u, reinterpret_cast<uint32_t *>(outr), lds};
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const Ray r = ray_new<F>(v3(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2]),
	                      v3(rays[i].direction[0], rays[i].direction[1], rays[i].direction[2]));
	float t;
	uint32_t prim;
	trace_closest<F, PRUNE>(S, S, SM, r, stk, t, prim);
	Hit h;
	uint32_t m;
	if (prim != kNoPrim) {
		make_hit<F>(S, prim, r, t, h, m);
		store_record(outr[i], h, m, prim, true);
	} else {
		make_sky_hit(S, h, m);
		store_record(outr[i], h, m, 0xFFFFFFFFFFFFFFFFull, true);
	}
}

template <bool PRUNE>
__global__ __launch_bounds__(256) void check_hit_index_kernel(const DevScene S, const DevRayDesc *__restrict__ rays,
                                                              const unsigned long long *__restrict__ object_index, uint64_t n,
                                                              DevHitRecord *__restrict__ outr)
{
	using F = FeatFull; // batch queries serve every scene: all primitive types compiled in
	extern __shared__ __align__(16) uint32_t lds[];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t *stk = lds + wave * (S.stack_depth * kStackStride) + lane;
	const StackMem SM = {S.stack_depth, 0u, reinterpret_cast<uint32_t *>(outr), lds}; // see check_hit_kernel
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const Ray r = ray_new<F>(v3(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2]),
	                      v3(rays[i].direction[0], rays[i].direction[1], rays[i].direction[2]));
	const uint32_t index = (uint32_t)object_index[i];
	const PrimGeom g = load_prim<F>(S, index);
	Hit h;
	h.t = 0.0f;
	h.point = h.error = h.normal = v3s(0.0f);
	h.uvx = h.uvy = 0.0f;
	h.has_uv = h.out = false;
	uint32_t m = 0;
	bool found = false;
	float lt;
	if (prim_t<F>(g, r, lt) && lt > 0.0f) {
		if (!trace_any<F, PRUNE>(S, S, SM, r, stk, lt, index)) {
			make_hit<F>(S, index, r, lt, h, m);
			found = true;
		}
	}
	store_record(outr[i], h, m, object_index[i], found);
}

#ifdef RT_STATS
// ---- diagnostic build only: a register-lean TRAVERSAL-ONLY persistent kernel (tests/probes/gpu_trace_queue.py).
// Lanes pull rays from a queue, walk the wide tree (NODE / LEAF voted as in the fine schedule), write (t, primitive) and
// refill in place.  It holds nothing but the ray, the best hit and the stack, so it can run at up to 8 waves/SIMD: the
// experiment behind DESIGN.md section 8.1 (what a wavefront split could give the big-tree configurations). ----
template <int WAVES>
__global__ __launch_bounds__(256, WAVES) void trace_queue_kernel(const DevScene S, const DevRayDesc *__restrict__ rays, uint32_t n, float2 *__restrict__ out,
                                                                 uint32_t *__restrict__ counter, unsigned long long *__restrict__ steps_out,
                                                                 uint32_t stack_cap, uint32_t ovf_depth, uint32_t *__restrict__ ovf)
{
	using F = Feat<true, true, false, false>;
	extern __shared__ __align__(16) uint32_t lds[];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	StackMem SM;
	SM.cap = stack_cap;
	SM.ovf_depth = ovf_depth;
	SM.ovf = ovf;
	SM.region = lds;
	uint32_t *stk = lds + wave * (stack_cap * kStackStride) + lane;
	enum { EMPTY = 0, NODE = 1, LEAF = 2, DONE = 3 };
	int ph = EMPTY;
	Ray ray;
	ray.o = ray.d = ray.inv = ray.shear = v3s(0.0f);
	uint32_t node = kRefDone, best_prim = kNoPrim, id = 0;
	int sp = 0;
	float best_t = 0.0f;
	unsigned long long n_steps = 0;
	uint32_t wq_next = 0, wq_end = 0;
	auto finish = [&]() {
		out[id] = make_float2(best_t, __uint_as_float(best_prim));
		ph = EMPTY;
	};
	for (;;) {
		const unsigned long long need = __ballot(ph == EMPTY);
		if (need != 0ull) {
			const uint32_t cnt = (uint32_t)__popcll(need), avail = wq_end - wq_next;
			uint32_t base = wq_end;
			if (avail < cnt) {
				const int leader = __ffsll((long long)need) - 1;
				uint32_t claimed = 0;
				if ((int)lane == leader)
					claimed = atomicAdd(counter, 64u);
				base = __shfl(claimed, leader);
			}
			if (ph == EMPTY) {
				const uint32_t r = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
				id = r < avail ? wq_next + r : base + (r - avail);
				if (id >= n) {
					ph = DONE;
				} else {
					ray = ray_new<F>(v3(rays[id].origin[0], rays[id].origin[1], rays[id].origin[2]),
					                 v3(rays[id].direction[0], rays[id].direction[1], rays[id].direction[2]));
					best_t = 0.0f;
					best_prim = kNoPrim;
					sp = 0;
					node = S.root4_ref;
					ph = ref_is_leaf(node) ? LEAF : NODE;
				}
			}
			if (avail < cnt) {
				wq_next = base + (cnt - avail);
				wq_end = base + 64u;
			} else {
				wq_next += cnt;
			}
		}
		const uint32_t c_node = (uint32_t)__popcll(__ballot(ph == NODE)), c_leaf = (uint32_t)__popcll(__ballot(ph == LEAF));
		if (c_node + c_leaf == 0u) {
			if (__ballot(ph == EMPTY) == 0ull)
				break;
			continue;
		}
		if (c_leaf >= kDrainLanes || c_node == 0u) {
			if (ph == LEAF) {
				uint32_t leaf_ref;
				if (wide_leaf_hit(S, node, ray, leaf_ref))
					closest_in_leaf<F>(S, ray, leaf_ref, best_t, best_prim);
				if (sp == 0) {
					finish();
				} else {
					--sp;
					node = ovf_depth == 0u ? stack_load<false>(SM, stk, sp) : stack_load<true>(SM, stk, sp);
					ph = ref_is_leaf(node) ? LEAF : NODE;
				}
			}
		} else {
#pragma unroll 1
			for (int step = 0; step < kNodeStepsPerVote; ++step) {
				if (ph == NODE) {
					n_steps += 1;
					if (ovf_depth == 0u)
						node = descend4<true, false>(S, SM, ray, node, stk, sp, best_prim != kNoPrim, best_t);
					else
						node = descend4<true, true>(S, SM, ray, node, stk, sp, best_prim != kNoPrim, best_t);
					if (node == kRefDone)
						finish();
					else if (ref_is_leaf(node))
						ph = LEAF;
				}
			}
		}
	}
	for (int off = 32; off > 0; off >>= 1)
		n_steps += __shfl_down(n_steps, off);
	if (lane == 0u)
		atomicAdd(steps_out, n_steps);
}

hipError_t launch_trace_queue(int waves, uint32_t n_blocks, size_t lds_bytes, hipStream_t stream, const DevScene &S, const void *rays, uint32_t n, void *out,
                              uint32_t *counter, unsigned long long *steps, uint32_t cap, uint32_t ovf_depth, uint32_t *ovf)
{
#define RT_TQ(W) \
	if (waves == W) { \
		hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(trace_queue_kernel<W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); \
		if (e_ != hipSuccess) \
			return e_; \
		hipLaunchKernelGGL(trace_queue_kernel<W>, dim3(n_blocks), dim3(256), lds_bytes, stream, S, static_cast<const DevRayDesc *>(rays), n, \
		                   static_cast<float2 *>(out), counter, steps, cap, ovf_depth, ovf); \
		return hipGetLastError(); \
	}
	RT_TQ(3) RT_TQ(4) RT_TQ(5) RT_TQ(6) RT_TQ(8)
#undef RT_TQ
	return hipErrorInvalidValue;
}
#endif

hipError_t launch_check_hit(bool prune, hipStream_t stream, const DevScene &S, const void *rays, uint64_t n, void *out)
{
	const size_t lds_bytes = four_wave_stack_lds_bytes(S);
	const uint32_t blocks = (uint32_t)((n + 255) / 256);
	// deep trees: more than the default 64 KB of dynamic LDS per workgroup (the whole worst-case stack lives in LDS here)
	hipError_t e = hipFuncSetAttribute(prune ? reinterpret_cast<const void *>(check_hit_kernel<true>) : reinterpret_cast<const void *>(check_hit_kernel<false>),
	                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	if (prune)
		hipLaunchKernelGGL(check_hit_kernel<true>, dim3(blocks), dim3(256), lds_bytes, stream, S,
		                   static_cast<const DevRayDesc *>(rays), n, static_cast<DevHitRecord *>(out));
	else
		hipLaunchKernelGGL(check_hit_kernel<false>, dim3(blocks), dim3(256), lds_bytes, stream, S,
		                   static_cast<const DevRayDesc *>(rays), n, static_cast<DevHitRecord *>(out));
	return hipGetLastError();
}

hipError_t launch_check_hit_index(bool prune, hipStream_t stream, const DevScene &S, const void *rays, const void *object_index,
                                  uint64_t n, void *out)
{
	const size_t lds_bytes = four_wave_stack_lds_bytes(S);
	const uint32_t blocks = (uint32_t)((n + 255) / 256);
	hipError_t e = hipFuncSetAttribute(prune ? reinterpret_cast<const void *>(check_hit_index_kernel<true>)
	                                         : reinterpret_cast<const void *>(check_hit_index_kernel<false>),
	                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	if (prune)
		hipLaunchKernelGGL(check_hit_index_kernel<true>, dim3(blocks), dim3(256), lds_bytes, stream, S,
		                   static_cast<const DevRayDesc *>(rays), static_cast<const unsigned long long *>(object_index), n,
		                   static_cast<DevHitRecord *>(out));
	else
		hipLaunchKernelGGL(check_hit_index_kernel<false>, dim3(blocks), dim3(256), lds_bytes, stream, S,
		                   static_cast<const DevRayDesc *>(rays), static_cast<const unsigned long long *>(object_index), n,
		                   static_cast<DevHitRecord *>(out));
	return hipGetLastError();
}

} // namespace rt
