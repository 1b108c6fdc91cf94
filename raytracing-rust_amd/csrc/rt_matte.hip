// rt_matte.hip -- anti-aliased ID mattes (rt_render_matte, rt_matte_extract, include/rt_hip.h): per pixel the most-covering
// primitive or material IDs of ALL passes with their coverage fractions (the Cryptomatte form), and the matte of a selection of IDs.
// Integer work throughout, one IEEE division per value written; tests/matte_checker.py restates it in numpy.
//
// matte_kernel<PRUNE> has the shape of aov_kernel (rt_aov.hip): one wave per 8 x 8 tile, one lane per pixel, the traversal stack
// in LDS, each lane loops over its passes -- the camera ray of rt_aov_common.h, one walk, and of the hit only the primitive slot:
// no Hit record, no material or texture evaluation.  The per-pixel table is eight IDs and eight counts in REGISTERS: every access
// is a fully unrolled compare / select over constant indices (a dynamic index would put the table in scratch).  Occupied slots are
// a prefix of the table, so "the slot that holds the ID, else the first free one" is the first slot that is free or matches.  The
// ranking is a fixed 19-exchange network over the keys count << 32 | ~id, descending: count first, then the smaller ID, an
// empty slot (key 0) last -- where it reads back as (UINT32_MAX, +0).  One store per layer per channel; a wave's stores are eight
// 32-byte row segments of its tile.
//
// matte_extract_kernel<STAGED>: one lane per pixel, the K (id, coverage) pairs of the pixel read coalesced, a binary search of the
// ascending selection per layer of positive coverage.  The search is bounded by n_sel alone, so an unsorted list costs wrong
// answers, never an access out of bounds.  A selection of at most kMatteStagedIds is copied to LDS first.
#include "rt_aov_common.h"
#include "rt_matte.h"

namespace rt {

struct MatteArgs {
	DevScene S;
	DevMatteParams P;
};

namespace {

constexpr uint32_t kMatteStagedIds = 2048u; // 8 KB of LDS per workgroup

struct MatteTable {
	uint32_t id[kMatteSlots], count[kMatteSlots];

	__device__ __forceinline__ MatteTable()
	{
#pragma unroll
		for (uint32_t s = 0; s < kMatteSlots; ++s) {
			id[s] = 0xFFFFFFFFu;
			count[s] = 0u;
		}
	}
	// one pass: the count of `v` goes up, or `v` takes the first free slot, or (table full) the pass is overflow, counted nowhere
	__device__ __forceinline__ void add(uint32_t v)
	{
		bool placed = false;
#pragma unroll
		for (uint32_t s = 0; s < kMatteSlots; ++s) {
			const bool here = !placed && (count[s] == 0u || id[s] == v);
			id[s] = here ? v : id[s];
			count[s] += here ? 1u : 0u;
			placed = placed || here;
		}
	}
};

__device__ __forceinline__ void exchange_descending(uint64_t &a, uint64_t &b)
{
	const uint64_t hi = a < b ? b : a, lo = a < b ? a : b;
	a = hi;
	b = lo;
}

// lower bound of `v` in sel[0, n): every index read is < n whatever the order of sel
template <class Ptr> __device__ __forceinline__ bool selected(Ptr sel, uint32_t n, uint32_t v)
{
	uint32_t lo = 0u, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (sel[mid] < v)
			lo = mid + 1u;
		else
			hi = mid;
	}
	return lo < n && sel[lo] == v;
}

} // namespace

template <bool PRUNE>
__global__ __launch_bounds__(256, 4) void matte_kernel(const MatteArgs args_by_value)
{
	using F = FeatFull; // every primitive type compiled in (as the AOV passes)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const DevAovParams &P = args_by_value.P.A;
	AovLane L;
	if (!aov_lane(S, P, lds, L))
		return;

	MatteTable table;
#pragma unroll 1
	for (uint32_t p = 0; p < P.spp; ++p) {
		const KArgPtr<MatteArgs> k = aov_kargs(args_by_value);
		const Ray ray = aov_camera_ray<F>(&k->P.A, L, p);
		float best_t;
		uint32_t prim;
		trace_closest<F, PRUNE>(S, S, L.SM, ray, L.stk, best_t, prim);
		uint32_t id = 0xFFFFFFFFu; // the sky is an ID like any other
		if (prim != kNoPrim) {
			if (k->P.id_kind == 0u) { // RT_MATTE_ID_PRIMITIVE: as the `primitive` channel of rt_render_aov
				const uint32_t *prim_desc = k->P.A.prim_desc;
				id = prim_desc != nullptr ? prim_desc[prim] : prim;
			} else { // the caller's material index, from the handle in the primitive record (rt_intersect.h load_prim)
				id = mat_handle_index(__float_as_uint(S.prims[prim].a[3]) >> 2);
			}
		}
		table.add(id);
	}

	uint64_t key[kMatteSlots];
#pragma unroll
	for (uint32_t s = 0; s < kMatteSlots; ++s)
		key[s] = table.count[s] != 0u ? ((uint64_t)table.count[s] << 32) | (uint32_t)~table.id[s] : 0ull;
	// a sorting network of 8 inputs, 19 exchanges in 6 layers
	exchange_descending(key[0], key[2]);
	exchange_descending(key[1], key[3]);
	exchange_descending(key[4], key[6]);
	exchange_descending(key[5], key[7]);
	exchange_descending(key[0], key[4]);
	exchange_descending(key[1], key[5]);
	exchange_descending(key[2], key[6]);
	exchange_descending(key[3], key[7]);
	exchange_descending(key[0], key[1]);
	exchange_descending(key[2], key[3]);
	exchange_descending(key[4], key[5]);
	exchange_descending(key[6], key[7]);
	exchange_descending(key[2], key[4]);
	exchange_descending(key[3], key[5]);
	exchange_descending(key[1], key[4]);
	exchange_descending(key[3], key[6]);
	exchange_descending(key[1], key[2]);
	exchange_descending(key[3], key[4]);
	exchange_descending(key[5], key[6]);

	const KArgPtr<MatteArgs> k = aov_kargs(args_by_value);
	const uint32_t layers = k->P.layers, spp = k->P.A.spp;
	const uint64_t n_px = (uint64_t)k->P.A.width * k->P.A.height;
	const float n = (float)spp;
	uint32_t *const ids = k->P.ids;
	float *const coverage = k->P.coverage;
	uint32_t written = 0u;
#pragma unroll
	for (uint32_t l = 0; l < kMatteSlots; ++l) {
		if (l < layers) { // (wave-uniform)
			const uint32_t count = (uint32_t)(key[l] >> 32);
			ids[l * n_px + L.pixel] = ~(uint32_t)key[l];
			coverage[l * n_px + L.pixel] = (float)count / n;
			written += count;
		}
	}
	float *const residual = k->P.residual;
	if (residual != nullptr)
		residual[L.pixel] = (float)(spp - written) / n;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void matte_extract_kernel(const DevMatteExtractParams P)
{
	__shared__ uint32_t s_sel[STAGED ? kMatteStagedIds : 1u];
	if (STAGED) {
		for (uint32_t i = threadIdx.x; i < P.n_sel; i += 256u)
			s_sel[i] = P.sel[i];
		__syncthreads();
	}
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	if (q >= P.n_px)
		return;
	uint32_t id[kMatteSlots];
	float c[kMatteSlots];
#pragma unroll
	for (uint32_t l = 0; l < kMatteSlots; ++l) {
		id[l] = 0u;
		c[l] = 0.0f;
		if (l < P.layers) {
			id[l] = P.ids[(uint64_t)l * P.n_px + q];
			c[l] = P.coverage[(uint64_t)l * P.n_px + q];
		}
	}
	float m = 0.0f;
#pragma unroll
	for (uint32_t l = 0; l < kMatteSlots; ++l) {
		if (l < P.layers && c[l] > 0.0f) { // an empty layer (coverage +0) matches nothing, the sky's ID included
			const bool in = STAGED ? selected(s_sel, P.n_sel, id[l]) : selected(P.sel, P.n_sel, id[l]);
			if (in)
				m = m + c[l];
		}
	}
	P.out[q] = fminf(m, 1.0f);
}

hipError_t launch_matte(bool prune, hipStream_t stream, const DevScene &S, const DevMatteParams &P)
{
	MatteArgs A;
	A.S = S;
	A.P = P;
	return launch_aov_tiles<MatteArgs>(matte_kernel<true>, matte_kernel<false>, prune, stream, P.A.n_tiles, A);
}

hipError_t launch_matte_extract(hipStream_t stream, const DevMatteExtractParams &P)
{
	const dim3 grid((P.n_px + 255u) / 256u), block(256);
	if (P.n_sel <= kMatteStagedIds)
		hipLaunchKernelGGL(matte_extract_kernel<true>, grid, block, 0, stream, P);
	else
		hipLaunchKernelGGL(matte_extract_kernel<false>, grid, block, 0, stream, P);
	return hipGetLastError();
}

} // namespace rt
