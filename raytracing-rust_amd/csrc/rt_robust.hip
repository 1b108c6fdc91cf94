// rt_robust.hip -- firefly-robust frames (rt_render_robust, rt_robust_combine, include/rt_hip.h): the S independent sums of a pixel
// that a render at sample_split = S leaves in the scene's partial buffer, or that a caller brings, ranked by luminance and
// averaged without the t lowest and the t highest.  The definition is in the header; tests/robust_checker.py restates it in
// numpy f32, bit for bit.
//
// Kernel (stable name for rocprofv3):
//   robust_chunk_kernel  one lane per work item of a chunk (= per pixel), 128 lanes per workgroup.  A wave reads 64 consecutive
//                        work items of one chunk: 768 contiguous bytes per load instruction triple, in both addressing modes.
//     pass 1   reads the S sums: the plain total, and per chunk the ordering key into the lane's LDS column keys[c][lane]
//              (consecutive lanes on consecutive banks: conflict-free, like the traversal stacks).  A private array indexed by
//              the chunk would live in scratch; the column does not.
//     ranks    eight chunks at a time held in registers, one sweep of the column per eight: r_c = #{k_j < k_c} + #{k_j == k_c,
//              j < c}, counted as (k_j <= k_c) before the block and (k_j < k_c) behind it.  The Gini sums A and B follow each
//              block in chunk order (l_c is recovered from its key); the ranks are parked in LDS four to a word.
//     pass 2   (only lanes that drop or trim something) reads the S sums again and adds those whose rank is kept, in chunk order.
//   Nothing synchronises: a lane touches its own column only.  S is padded to a multiple of eight with keys that rank last.
#include "rt_robust.h"
#include "rt_chunk_stats.h"

#include "../../include/rt_hip.h"

namespace rt {

namespace {

constexpr uint32_t kNotFinite = 0xFFFFFFFFu;
constexpr uint32_t T = kRobustBlockThreads;

} // namespace

__global__ __launch_bounds__(kRobustBlockThreads) void robust_chunk_kernel(const DevRobustParams P)
{
	extern __shared__ uint32_t robust_lds[];
	const uint32_t wp = blockIdx.x * T + threadIdx.x;
	if (wp >= P.n_work)
		return;
	size_t p = wp; // (the caller's planes: frame raster)
	if (P.tile_w != 0u) {
		if (!frame_work_pixel(wp, P.tile_w, P.tile_h, P.tiles_x, P.width, P.height, p))
			return; // edge-tile padding
	}
	const size_t p3 = 3u * p;
	const Demod d = demod_divisors(P.albedo, p3);
	const uint32_t S = P.split, Sp = (S + 7u) & ~7u;
	const float n = (float)P.chunk_passes;
	const float *const first = P.sums + 3u * (size_t)wp;
	const size_t stride = 3u * (size_t)P.n_work;
	uint32_t *const keys = robust_lds + threadIdx.x;           // [Sp][T]
	uint32_t *const ranks = robust_lds + Sp * T + threadIdx.x; // [Sp / 4][T], four ranks to a word

	// ---- pass 1: the plain total, the keys, S_f ----
	float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
	uint32_t sf = 0u;
	for (uint32_t c = 0; c < S; ++c) {
		const float *m = first + c * stride;
		const float m0 = m[0], m1 = m[1], m2 = m[2];
		t0 = t0 + m0;
		t1 = t1 + m1;
		t2 = t2 + m2;
		const float l = chunk_lum(m, n, d);
		const uint32_t b = __float_as_uint(l);
		uint32_t k = kNotFinite;
		if (__builtin_isfinite(l)) {
			k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
			++sf;
		}
		keys[c * T] = k;
	}
	for (uint32_t c = S; c < Sp; ++c)
		keys[c * T] = kNotFinite; // padding: ranks behind every chunk (ties go to the lower index)

	// ---- ranks, and the Gini sums over the finite chunks in chunk order ----
	const int32_t sf_less_1 = (int32_t)sf - 1;
	float A = 0.0f, B = 0.0f;
	for (uint32_t c0 = 0; c0 < Sp; c0 += 8u) {
		uint32_t kc[8], r[8];
#pragma unroll
		for (uint32_t u = 0; u < 8u; ++u) {
			kc[u] = keys[(c0 + u) * T];
			r[u] = 0u;
		}
		for (uint32_t j = 0; j < c0; ++j) {
			const uint32_t kj = keys[j * T];
#pragma unroll
			for (uint32_t u = 0; u < 8u; ++u)
				r[u] += kj <= kc[u] ? 1u : 0u;
		}
#pragma unroll
		for (uint32_t v = 0; v < 8u; ++v) {
#pragma unroll
			for (uint32_t u = 0; u < 8u; ++u) {
				if (v < u)
					r[u] += kc[v] <= kc[u] ? 1u : 0u;
				else if (v > u)
					r[u] += kc[v] < kc[u] ? 1u : 0u;
			}
		}
		for (uint32_t j = c0 + 8u; j < Sp; ++j) {
			const uint32_t kj = keys[j * T];
#pragma unroll
			for (uint32_t u = 0; u < 8u; ++u)
				r[u] += kj < kc[u] ? 1u : 0u;
		}
#pragma unroll
		for (uint32_t u = 0; u < 8u; ++u) {
			if (kc[u] != kNotFinite) {
				const float l = __uint_as_float((kc[u] & 0x80000000u) ? (kc[u] & 0x7FFFFFFFu) : ~kc[u]);
				A = A + (float)(2 * (int32_t)r[u] - sf_less_1) * l;
				B = B + l;
			}
		}
		ranks[(c0 / 4u) * T] = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
		ranks[(c0 / 4u + 1u) * T] = r[4] | (r[5] << 8) | (r[6] << 16) | (r[7] << 24);
	}
	const float G = A / ((float)sf * B);
	const float g = G > 0.0f ? fminf(G, 1.0f) : 0.0f; // fminf(fmaxf(G, 0), 1) with fmaxf(-0, +0) pinned to +0; a NaN G gives 0

	// ---- the trim count ----
	const uint32_t tmax = sf ? (sf - 1u) / 2u : 0u;
	uint32_t t = tmax; // RT_ROBUST_MEDIAN
	if (P.mode == RT_ROBUST_TRIM)
		t = P.trim < tmax ? P.trim : tmax;
	else if (P.mode == RT_ROBUST_GINI)
		t = (uint32_t)fminf(g * P.gini_gain * (float)tmax, (float)tmax);

	// ---- pass 2: the kept sums in chunk order.  With nothing dropped and nothing trimmed the kept sum is the plain total ----
	float o0 = t0, o1 = t1, o2 = t2;
	uint32_t divisor = S * P.chunk_passes;
	if (sf != 0u && (t != 0u || sf != S)) {
		const uint32_t hi = sf - t; // kept: t <= r_c < S_f - t (which implies finite: the finite chunks hold the ranks below S_f)
		o0 = o1 = o2 = 0.0f;
		for (uint32_t c0 = 0; c0 < S; c0 += 4u) {
			const uint32_t word = ranks[(c0 / 4u) * T];
#pragma unroll
			for (uint32_t u = 0; u < 4u; ++u) {
				const uint32_t c = c0 + u, rc = (word >> (8u * u)) & 0xFFu;
				if (c < S && rc >= t && rc < hi) {
					const float *m = first + c * stride;
					o0 = o0 + m[0];
					o1 = o1 + m[1];
					o2 = o2 + m[2];
				}
			}
		}
		divisor = (sf - 2u * t) * P.chunk_passes;
	}
	const float dv = (float)divisor;
	P.out[p3] = o0 / dv;
	P.out[p3 + 1u] = o1 / dv;
	P.out[p3 + 2u] = o2 / dv;
	if (P.mean) {
		const float all = (float)(S * P.chunk_passes);
		P.mean[p3] = t0 / all;
		P.mean[p3 + 1u] = t1 / all;
		P.mean[p3 + 2u] = t2 / all;
	}
	if (P.gini)
		P.gini[p] = g;
	if (P.trimmed)
		P.trimmed[p] = (uint8_t)t;
	if (P.dropped)
		P.dropped[p] = (uint8_t)(S - sf);
}

hipError_t launch_robust_chunks(hipStream_t stream, const DevRobustParams &P)
{
	const uint32_t padded = (P.split + 7u) & ~7u;
	const size_t lds_bytes = (size_t)padded * T * 5u; // the keys, and a byte per rank
	hipLaunchKernelGGL(robust_chunk_kernel, dim3((P.n_work + T - 1u) / T), dim3(T), lds_bytes, stream, P);
	return hipGetLastError();
}

} // namespace rt
