// rt_bloom.hip -- the bloom stage (rt_bloom, include/rt_hip.h): the over-threshold part of a W x H RGB float frame, blurred wide by
// a pyramid of 2:1 reductions and expansions, added back to the frame.  The arithmetic is defined in the header;
// tests/bloom_checker.py restates it in numpy bit for bit.
//
// Launch sequence (launch_bloom), on one stream, for n levels (2n launches without the fused tail):
//   bloom_reduce<true>    bright pass + reduce, frame -> level 0.  A 256-thread workgroup makes a 32 x 8 tile of the level: it stages
//                         the 66 x 18 source footprint (indices clamped to the image, the bright pass applied on the way) in LDS,
//                         runs the horizontal pass into LDS (32 x 18) and the vertical pass out of it.  The full-resolution bright
//                         image never exists.  Capped grid, grid-stride over the tiles.
//   bloom_reduce<false>   level i-1 -> level i, the same without the bright pass
//   bloom_tail            fuse_tail: ONE 1024-thread workgroup reduces level t-1 into the levels t .. n-1, all of them in LDS
//                         (bloom_levels, rt_bloom.h, picks t), expands and accumulates them back up in LDS and writes U_t alone
//   bloom_expand_add      U_i = B_i + scatter * E(U_{i+1}) in place over B_i: one lane per pixel of level i, four taps of level i+1
//   bloom_composite       out = c + (intensity * E(U_0)) / s: the last expand, one lane per pixel of the frame
// The exposure scale s = 2^ev is computed by one lane per workgroup from the display state ON THE DEVICE (bloom_reduce<true> and
// bloom_composite), so a captured graph follows the display's adaptation.  Nothing needs a clear: every level pixel is written
// before it is read.
#include <algorithm>
#include <cfloat>

#include "rt_bloom.h"
#include "rt_post_common.h"
#include "../../include/rt_detmath.h"

namespace rt {

namespace {

constexpr uint32_t kFootW = 2u * kBloomTileW + 2u, kFootH = 2u * kBloomTileH + 2u; // source pixels under one tile

__device__ inline float bloom_scale(const DevBloomParams &P)
{
	const float ev = P.state ? P.state->ev + P.exposure_ev : P.exposure_ev;
	return rt_powf(2.0f, ev);
}

// the bright pass of one source pixel, in place
__device__ inline void bright_px(const DevBloomParams &P, float s, float &r, float &g, float &b)
{
	float x[3] = {r, g, b};
#pragma unroll
	for (int i = 0; i < 3; ++i) {
		const float a = (__builtin_isfinite(x[i]) && x[i] > 0.0f) ? x[i] : 0.0f;
		x[i] = fminf(a * s, FLT_MAX);
	}
	float Y = lum(x[0], x[1], x[2]);
	if (Y > P.clamp_max) {
		const float c = P.clamp_max / Y;
#pragma unroll
		for (int i = 0; i < 3; ++i)
			x[i] = x[i] * c;
		Y = P.clamp_max;
	}
	const float k = P.threshold * P.knee;
	const float q = fminf(fmaxf((Y - P.threshold) + k, 0.0f), 2.0f * k);
	const float soft = (q * q) / (4.0f * k + 1e-5f);
	const float wgt = fmaxf(soft, Y - P.threshold) / fmaxf(Y, 1e-5f);
	r = x[0] * wgt;
	g = x[1] * wgt;
	b = x[2] * wgt;
}

__device__ inline float reduce4(float a, float b, float c, float d) { return ((a * 0.125f + b * 0.375f) + c * 0.375f) + d * 0.125f; }

__device__ inline uint32_t clamp_index(long long i, uint32_t n) { return i < 0 ? 0u : (i >= (long long)n ? n - 1u : (uint32_t)i); }

// pixel (X, Y) of the reduction of the w x h RGB image at `img` (global memory or LDS), the definition taken literally: four
// horizontal sums, then the vertical one
__device__ inline void reduce_px(const float *img, uint32_t w, uint32_t h, uint32_t X, uint32_t Y, float out[3])
{
	uint32_t xi[4], yi[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		xi[k] = 3u * clamp_index(2ll * X - 1 + k, w);
		yi[k] = clamp_index(2ll * Y - 1 + k, h);
	}
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		float T[4];
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const float *row = img + (size_t)yi[j] * w * 3u + c;
			T[j] = reduce4(row[xi[0]], row[xi[1]], row[xi[2]], row[xi[3]]);
		}
		out[c] = reduce4(T[0], T[1], T[2], T[3]);
	}
}

// the two coarse taps of fine index X along one axis of n coarse pixels, in the order the definition adds them
__device__ inline void expand_taps(uint32_t X, uint32_t n, uint32_t &i0, uint32_t &i1, float &w0, float &w1)
{
	if ((X & 1u) == 0u) {
		i0 = X >= 2u ? X / 2u - 1u : 0u;
		i1 = X / 2u;
		w0 = 0.25f;
		w1 = 0.75f;
	} else {
		i0 = (X - 1u) / 2u;
		i1 = (X + 1u) / 2u < n ? (X + 1u) / 2u : n - 1u;
		w0 = 0.75f;
		w1 = 0.25f;
	}
}

// pixel (X, Y) of the expansion of the cw x ch RGB image at `img` (global memory or LDS): horizontal first, then vertical
__device__ inline void expand_px(const float *img, uint32_t cw, uint32_t ch, uint32_t X, uint32_t Y, float out[3])
{
	uint32_t i0, i1, j0, j1;
	float wx0, wx1, wy0, wy1;
	expand_taps(X, cw, i0, i1, wx0, wx1);
	expand_taps(Y, ch, j0, j1, wy0, wy1);
	const float *r0 = img + (size_t)j0 * cw * 3u, *r1 = img + (size_t)j1 * cw * 3u;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const float h0 = r0[3ull * i0 + c] * wx0 + r0[3ull * i1 + c] * wx1;
		const float h1 = r1[3ull * i0 + c] * wx0 + r1[3ull * i1 + c] * wx1;
		out[c] = h0 * wy0 + h1 * wy1;
	}
}

} // namespace

// src (sw x sh; the frame when BRIGHT) -> dst (dw x dh = ceil(sw/2) x ceil(sh/2))
template <bool BRIGHT>
__global__ __launch_bounds__(256) void bloom_reduce(const DevBloomParams P, const float *__restrict__ src, uint32_t sw, uint32_t sh,
                                                    float *__restrict__ dst, uint32_t dw, uint32_t dh, uint32_t tiles_x, uint32_t n_tiles)
{
	__shared__ float s_src[3][kFootH][kFootW];
	__shared__ float s_t[3][kFootH][kBloomTileW];
	__shared__ float s_scale;
	const uint32_t t = threadIdx.x;
	float s = 1.0f;
	if (BRIGHT) {
		if (t == 0)
			s_scale = bloom_scale(P);
		__syncthreads();
		s = s_scale;
	}
	for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
		const uint32_t X0 = tx * kBloomTileW, Y0 = ty * kBloomTileH;
		// the footprint: local (li, lj) is source pixel (2 X0 - 1 + li, 2 Y0 - 1 + lj), clamped to the image; lanes run along rows
		for (uint32_t i = t; i < kFootW * kFootH; i += 256u) {
			const uint32_t lj = i / kFootW, li = i - lj * kFootW;
			const uint32_t gx = clamp_index(2ll * X0 - 1 + li, sw), gy = clamp_index(2ll * Y0 - 1 + lj, sh);
			const float *px = src + ((size_t)gy * sw + gx) * 3u;
			float r = px[0], g = px[1], b = px[2];
			if (BRIGHT)
				bright_px(P, s, r, g, b);
			s_src[0][lj][li] = r;
			s_src[1][lj][li] = g;
			s_src[2][lj][li] = b;
		}
		__syncthreads();
		for (uint32_t i = t; i < 3u * kFootH * kBloomTileW; i += 256u) { // horizontal: output column lx of footprint row (c, lj)
			const uint32_t row = i / kBloomTileW, lx = i - row * kBloomTileW;
			const float *f = &s_src[0][0][0] + row * kFootW + 2u * lx;
			(&s_t[0][0][0])[i] = reduce4(f[0], f[1], f[2], f[3]);
		}
		__syncthreads();
		const uint32_t lx = t & (kBloomTileW - 1u), ly = t / kBloomTileW;
		const uint32_t X = X0 + lx, Y = Y0 + ly;
		if (X < dw && Y < dh) {
			float *o = dst + ((size_t)Y * dw + X) * 3u;
#pragma unroll
			for (int c = 0; c < 3; ++c)
				o[c] = reduce4(s_t[c][2u * ly][lx], s_t[c][2u * ly + 1u][lx], s_t[c][2u * ly + 2u][lx], s_t[c][2u * ly + 3u][lx]);
		}
		__syncthreads(); // the next trip overwrites both arrays
	}
}

// The fused tail: src (sw x sh, level t-1 in the workspace) is reduced into m levels held in LDS one after the other, the levels
// are expanded and accumulated from the smallest up, and the first (U_t) is written to dst.  One workgroup; the per-pixel
// arithmetic is reduce_px / expand_px, what the tiled kernels compute, so the bytes are theirs.
__global__ __launch_bounds__(1024) void bloom_tail(const float *__restrict__ src, uint32_t sw, uint32_t sh, uint32_t m, float scatter,
                                                   float *__restrict__ dst)
{
	__shared__ float lv[3u * kBloomTailPixels];
	const uint32_t t = threadIdx.x;
	const uint32_t w0 = (sw + 1u) / 2u, h0 = (sh + 1u) / 2u;
	for (uint32_t p = t; p < w0 * h0; p += 1024u) {
		const uint32_t Y = p / w0, X = p - Y * w0;
		float v[3];
		reduce_px(src, sw, sh, X, Y, v);
		lv[3u * p] = v[0];
		lv[3u * p + 1u] = v[1];
		lv[3u * p + 2u] = v[2];
	}
	__syncthreads();
	uint32_t pw = w0, ph = h0, poff = 0u; // the level above the one being made, and where it starts (in pixels)
	for (uint32_t k = 1; k < m; ++k) {
		const uint32_t w = (pw + 1u) / 2u, h = (ph + 1u) / 2u, off = poff + pw * ph;
		for (uint32_t p = t; p < w * h; p += 1024u) {
			const uint32_t Y = p / w, X = p - Y * w;
			float v[3];
			reduce_px(lv + 3u * poff, pw, ph, X, Y, v);
			lv[3u * (off + p)] = v[0];
			lv[3u * (off + p) + 1u] = v[1];
			lv[3u * (off + p) + 2u] = v[2];
		}
		__syncthreads();
		pw = w;
		ph = h;
		poff = off;
	}
	for (uint32_t k = m - 1u; k-- > 0u;) { // U_k = B_k + scatter * E(U_{k+1}), in place
		uint32_t fw = w0, fh = h0, foff = 0u;
		for (uint32_t j = 0; j < k; ++j) {
			foff += fw * fh;
			fw = (fw + 1u) / 2u;
			fh = (fh + 1u) / 2u;
		}
		const uint32_t cw = (fw + 1u) / 2u, ch = (fh + 1u) / 2u, coff = foff + fw * fh;
		for (uint32_t p = t; p < fw * fh; p += 1024u) {
			const uint32_t Y = p / fw, X = p - Y * fw;
			float e[3];
			expand_px(lv + 3u * coff, cw, ch, X, Y, e);
			float *f = lv + 3u * (foff + p);
			f[0] = f[0] + scatter * e[0];
			f[1] = f[1] + scatter * e[1];
			f[2] = f[2] + scatter * e[2];
		}
		__syncthreads();
	}
	for (uint32_t i = t; i < 3u * w0 * h0; i += 1024u)
		dst[i] = lv[i];
}

// fine (fw x fh) = fine + scatter * E(coarse), coarse ceil(fw/2) x ceil(fh/2)
__global__ __launch_bounds__(256) void bloom_expand_add(float *__restrict__ fine, uint32_t fw, uint32_t fh, const float *__restrict__ coarse,
                                                        float scatter)
{
	const uint32_t n = fw * fh, cw = (fw + 1u) / 2u, ch = (fh + 1u) / 2u;
	const uint32_t stride = gridDim.x * 256u;
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += stride) {
		const uint32_t Y = p / fw, X = p - Y * fw;
		float e[3];
		expand_px(coarse, cw, ch, X, Y, e);
		float *f = fine + 3ull * p;
		f[0] = f[0] + scatter * e[0];
		f[1] = f[1] + scatter * e[1];
		f[2] = f[2] + scatter * e[2];
	}
}

// out = c + (intensity * E(U_0)) / s.  out may be the frame itself: a lane reads only its own pixel of it
__global__ __launch_bounds__(256) void bloom_composite(const DevBloomParams P, const float *__restrict__ u0, uint32_t cw, uint32_t ch)
{
	__shared__ float s_scale;
	if (threadIdx.x == 0)
		s_scale = bloom_scale(P);
	__syncthreads();
	const float s = s_scale;
	const uint32_t n = P.width * P.height, stride = gridDim.x * 256u;
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += stride) {
		const uint32_t Y = p / P.width, X = p - Y * P.width;
		float e[3];
		expand_px(u0, cw, ch, X, Y, e);
		const float *c = P.rgb + 3ull * p;
		const float r = c[0] + (P.intensity * e[0]) / s, g = c[1] + (P.intensity * e[1]) / s, b = c[2] + (P.intensity * e[2]) / s;
		float *o = P.out + 3ull * p;
		o[0] = r;
		o[1] = g;
		o[2] = b;
	}
}

hipError_t launch_bloom(hipStream_t stream, const DevBloomParams &P, const BloomLevels &L)
{
	auto plane = [&](uint32_t i) { return reinterpret_cast<float *>(P.ws + L.offset[i]); };
	auto blocks = [](uint64_t n_px) { return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>((n_px + 255u) / 256u, kBloomMaxBlocks)); };
	const uint32_t n = L.n, tail = P.fuse_tail ? L.tail_from : n; // levels tail .. n-1 are the fused tail's
	for (uint32_t i = 0; i < tail; ++i) {
		const uint32_t tiles_x = (L.w[i] + kBloomTileW - 1u) / kBloomTileW, n_tiles = tiles_x * ((L.h[i] + kBloomTileH - 1u) / kBloomTileH);
		const dim3 grid(std::min(n_tiles, kBloomMaxTiles));
		if (i == 0)
			hipLaunchKernelGGL(bloom_reduce<true>, grid, dim3(256), 0, stream, P, P.rgb, P.width, P.height, plane(0), L.w[0], L.h[0], tiles_x,
			                   n_tiles);
		else
			hipLaunchKernelGGL(bloom_reduce<false>, grid, dim3(256), 0, stream, P, plane(i - 1), L.w[i - 1], L.h[i - 1], plane(i), L.w[i],
			                   L.h[i], tiles_x, n_tiles);
	}
	if (tail < n)
		hipLaunchKernelGGL(bloom_tail, dim3(1), dim3(1024), 0, stream, plane(tail - 1), L.w[tail - 1], L.h[tail - 1], n - tail, P.scatter,
		                   plane(tail));
	for (uint32_t i = std::min(tail, n - 1u); i-- > 0u;) // the levels whose U is still B
		hipLaunchKernelGGL(bloom_expand_add, dim3(blocks((uint64_t)L.w[i] * L.h[i])), dim3(256), 0, stream, plane(i), L.w[i], L.h[i],
		                   plane(i + 1), P.scatter);
	hipLaunchKernelGGL(bloom_composite, dim3(blocks((uint64_t)P.width * P.height)), dim3(256), 0, stream, P, plane(0), L.w[0], L.h[0]);
	return hipGetLastError();
}

} // namespace rt
