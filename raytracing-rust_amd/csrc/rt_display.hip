// rt_display.hip -- the display stage (rt_display, include/rt_hip.h): a luminance histogram, metered auto-exposure with eye
// adaptation, a tone curve, an output transfer function and 8-bit quantisation of a W x H RGB float frame.  The arithmetic is
// defined in the header; tests/display_checker.py restates it in numpy bit for bit.
//
// Launch sequence (launch_display), on one stream:
//   display_histogram   256-thread workgroups over a capped grid (grid-stride): four pixels per lane per step as three float4 loads
//                       where the input is 16-byte aligned; one 256-bin sub-histogram per wave in LDS (ds atomics); each workgroup
//                       writes its 256 counts to its row of the workspace with ordinary stores (no global atomics, no memset)
//   display_exposure    one 1024-thread workgroup: the rows summed per bin, an inclusive prefix in LDS, the overlap weights per bin,
//                       then one lane meters in bin order in f64, adapts, updates the state and leaves 2^ev and the dither frame
//                       in the workspace for the map kernel (no host round trip)
//   display_map         exposure, tone curve, transfer and quantisation: four pixels per lane (three float4 loads, one 16-byte store
//                       for RGBA8 / BGRA8, 12 bytes for RGB8), or one pixel per lane for unaligned buffers
#include <algorithm>

#include "rt_display.h"
#include "rt_post_common.h"
#include "../../include/rt_detmath.h"

namespace rt {

namespace {

// log2(1 + (m + 0.5) / 8): the centre of sub-bin m of an octave (include/rt_hip.h)
__constant__ const float kLog2Mid[8] = {0.0874628413f, 0.247927513f, 0.392317423f, 0.523561956f,
                                        0.643856190f,  0.754887502f, 0.857980995f, 0.954196310f};

// the histogram bin of a metered pixel, -1 for one that is not metered
__device__ inline int display_bin(float r, float g, float b)
{
	const float y = lum(r, g, b);
	if (!(__builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b) && __builtin_isfinite(y) && y > 0.0f))
		return -1;
	const int k = (int)(__float_as_uint(y) >> 20) - 888;
	return k < 0 ? 0 : (k > 255 ? 255 : k);
}

__device__ inline uint32_t sat_u8(float q) { return !(q > 0.0f) ? 0u : (q >= 255.0f ? 255u : (uint32_t)q); }

// one pixel: the three bytes r | g << 8 | b << 16
__device__ inline uint32_t display_px(const DevDisplayParams &P, float s, uint32_t frame, uint32_t x, uint32_t y, float r, float g,
                                      float b)
{
	float c[3] = {r * s, g * s, b * s};
	if (P.tonemap == RT_TONEMAP_REINHARD) {
		const float Y = lum(c[0], c[1], c[2]);
		if (Y > 0.0f && __builtin_isfinite(Y)) {
			const float k = ((Y * (1.0f + Y / P.white2)) / (1.0f + Y)) / Y;
			for (int i = 0; i < 3; ++i)
				c[i] = c[i] * k;
		}
	} else if (P.tonemap == RT_TONEMAP_ACES) {
		for (int i = 0; i < 3; ++i) {
			const float v = c[i];
			c[i] = (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f);
		}
	} else if (P.tonemap == RT_TONEMAP_HABLE) {
		for (int i = 0; i < 3; ++i)
			c[i] = display_hable(c[i]) / P.hable_fw;
	}
	float u[3] = {0.0f, 0.0f, 0.0f};
	if (P.quantiser == RT_QUANT_DITHER) {
		uint32_t w[4] = {x, y, frame, 0u};
		rt_philox4x32_10(w, P.seed_lo, P.seed_hi);
		for (int i = 0; i < 3; ++i)
			u[i] = (float)(w[i] >> 8) * 0x1p-24f;
	}
	uint32_t bytes = 0;
	for (int i = 0; i < 3; ++i) {
		float t = fminf(fmaxf(c[i], 0.0f), 1.0f);
		if (P.transfer == RT_TRANSFER_SRGB)
			t = t <= 0.0031308f ? 12.92f * t : 1.055f * rt_powf(t, 1.0f / 2.4f) - 0.055f;
		else if (P.transfer == RT_TRANSFER_GAMMA)
			t = rt_powf(t, P.inv_gamma);
		uint32_t q;
		if (P.quantiser == RT_QUANT_ROUND)
			q = sat_u8(t * 255.0f + 0.5f);
		else if (P.quantiser == RT_QUANT_DITHER)
			q = sat_u8(floorf(t * 255.0f + u[i]));
		else
			q = sat_u8(t * 255.999f);
		bytes |= q << (8 * i);
	}
	return bytes;
}

// RGBA8 / BGRA8 word of a pixel
__device__ inline uint32_t word4(int format, uint32_t rgb)
{
	if (format == RT_PIXEL_BGRA8)
		rgb = ((rgb & 0xFFu) << 16) | (rgb & 0xFF00u) | ((rgb >> 16) & 0xFFu);
	return rgb | 0xFF000000u;
}

} // namespace

template <bool kAligned> __global__ __launch_bounds__(256) void display_histogram(const DevDisplayParams P)
{
	__shared__ uint32_t sub[4][kDisplayBins];
	const uint32_t t = threadIdx.x;
	for (uint32_t i = 0; i < 4; ++i)
		sub[i][t] = 0u;
	__syncthreads();
	uint32_t *h = sub[t >> 6];
	auto add = [h](float r, float g, float b) {
		const int k = display_bin(r, g, b);
		if (k >= 0)
			atomicAdd(&h[k], 1u);
	};
	const uint32_t stride = gridDim.x * 256u, gid = blockIdx.x * 256u + t;
	if (kAligned) {
		const float4 *v = reinterpret_cast<const float4 *>(P.rgb);
		const uint32_t n_quads = P.n_px / 4u;
		uint32_t q = gid;
		for (; q + stride < n_quads; q += 2u * stride) { // two quads per step: six loads in flight before the first atomic
			const size_t a = 3ull * q, c = 3ull * (q + stride);
			const float4 a0 = v[a], a1 = v[a + 1], a2 = v[a + 2], c0 = v[c], c1 = v[c + 1], c2 = v[c + 2];
			add(a0.x, a0.y, a0.z);
			add(a0.w, a1.x, a1.y);
			add(a1.z, a1.w, a2.x);
			add(a2.y, a2.z, a2.w);
			add(c0.x, c0.y, c0.z);
			add(c0.w, c1.x, c1.y);
			add(c1.z, c1.w, c2.x);
			add(c2.y, c2.z, c2.w);
		}
		if (q < n_quads) {
			const size_t a = 3ull * q;
			const float4 a0 = v[a], a1 = v[a + 1], a2 = v[a + 2];
			add(a0.x, a0.y, a0.z);
			add(a0.w, a1.x, a1.y);
			add(a1.z, a1.w, a2.x);
			add(a2.y, a2.z, a2.w);
		}
		if (blockIdx.x == 0 && t < (P.n_px & 3u)) {
			const size_t p3 = 3ull * (4ull * n_quads + t);
			add(P.rgb[p3], P.rgb[p3 + 1], P.rgb[p3 + 2]);
		}
	} else {
		for (uint32_t p = gid; p < P.n_px; p += stride) {
			const size_t p3 = 3ull * p;
			add(P.rgb[p3], P.rgb[p3 + 1], P.rgb[p3 + 2]);
		}
	}
	__syncthreads();
	uint32_t *row = reinterpret_cast<uint32_t *>(P.ws + kDisplayParamBytes) + (size_t)blockIdx.x * kDisplayBins;
	row[t] = sub[0][t] + sub[1][t] + sub[2][t] + sub[3][t];
}

__global__ __launch_bounds__(1024) void display_exposure(const DevDisplayParams P, uint32_t rows)
{
	__shared__ uint32_t part[16][kDisplayBins];
	__shared__ uint32_t cum[kDisplayBins];
	__shared__ double ow[kDisplayBins], pw[kDisplayBins];
	const uint32_t t = threadIdx.x, g = t & 63u, r0 = t >> 6;
	// 16 groups of 64 lanes; lane g of group r0 sums bins 4g .. 4g+3 over rows r0, r0 + 16, ... (integer sums: any order)
	const uint4 *src = reinterpret_cast<const uint4 *>(P.ws + kDisplayParamBytes);
	uint4 acc = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 4
	for (uint32_t r = r0; r < rows; r += 16u) {
		const uint4 v = src[(size_t)r * (kDisplayBins / 4) + g];
		acc.x += v.x;
		acc.y += v.y;
		acc.z += v.z;
		acc.w += v.w;
	}
	part[r0][4u * g] = acc.x;
	part[r0][4u * g + 1u] = acc.y;
	part[r0][4u * g + 2u] = acc.z;
	part[r0][4u * g + 3u] = acc.w;
	__syncthreads();
	uint32_t n = 0;
	if (t < kDisplayBins) {
		for (int k = 0; k < 16; ++k)
			n += part[k][t];
		cum[t] = n;
		if (P.histogram)
			P.histogram[t] = n;
	}
	__syncthreads();
	for (uint32_t off = 1; off < kDisplayBins; off <<= 1) { // inclusive prefix (Hillis-Steele)
		uint32_t v = 0;
		if (t < kDisplayBins && t >= off)
			v = cum[t - off];
		__syncthreads();
		if (t < kDisplayBins)
			cum[t] += v;
		__syncthreads();
	}
	if (t < kDisplayBins) { // bin t covers ranks [cum - n, cum); its weight is the overlap with [lo, hi)
		const double total = (double)cum[kDisplayBins - 1];
		const double lo = floor(total * (double)P.meter_low), hi = ceil(total * (double)P.meter_high);
		const double c0 = (double)(cum[t] - n), c1 = (double)cum[t];
		const double o = fmax(0.0, fmin(c1, hi) - fmax(c0, lo));
		const double lambda = (double)((int)(t >> 3) - 16) + (double)kLog2Mid[t & 7u];
		ow[t] = o;
		pw[t] = o * lambda;
	}
	__syncthreads();
	if (t != 0)
		return;
	double num = 0.0, den = 0.0;
	for (uint32_t b = 0; b < kDisplayBins; ++b) { // in bin order
		den = den + ow[b];
		num = num + pw[b];
	}
	float metered = __builtin_nanf(""), target = P.exposure_ev;
	if (den > 0.0) {
		metered = (float)(num / den);
		if (P.mode == RT_EXPOSURE_AUTO)
			target = fminf(fmaxf(P.key_ev - metered, P.ev_min), P.ev_max) + P.exposure_ev;
	}
	float ev = target;
	uint32_t frame = 0;
	if (P.state) {
		const float prev = P.state->ev;
		frame = P.state->frames;
		if (frame > 0u && P.adaptation != 1.0f)
			ev = prev + P.adaptation * (target - prev);
		P.state->ev = ev;
		P.state->frames = frame == 0xFFFFFFFFu ? frame : frame + 1u;
		P.state->metered = metered;
	}
	reinterpret_cast<float *>(P.ws)[0] = rt_powf(2.0f, ev);
	reinterpret_cast<uint32_t *>(P.ws)[1] = frame;
}

template <bool kAligned> __global__ __launch_bounds__(256) void display_map(const DevDisplayParams P)
{
	const float s = reinterpret_cast<const float *>(P.ws)[0];
	const uint32_t frame = reinterpret_cast<const uint32_t *>(P.ws)[1];
	const uint32_t W = P.width, stride = gridDim.x * 256u, gid = blockIdx.x * 256u + threadIdx.x;
	const bool rgb8 = P.format == RT_PIXEL_RGB8;
	if (kAligned) {
		const float4 *v = reinterpret_cast<const float4 *>(P.rgb);
		const uint32_t n_quads = P.n_px / 4u;
		for (uint32_t q = gid; q < n_quads; q += stride) {
			const size_t a = 3ull * q;
			const float4 a0 = v[a], a1 = v[a + 1], a2 = v[a + 2];
			uint32_t y = (4u * q) / W, x = 4u * q - y * W;
			uint32_t px[4];
			const float f[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				px[k] = display_px(P, s, frame, x, y, f[3 * k], f[3 * k + 1], f[3 * k + 2]);
				if (++x == W) {
					x = 0;
					++y;
				}
			}
			if (rgb8) {
				uint3 o;
				o.x = px[0] | (px[1] << 24);
				o.y = (px[1] >> 8) | (px[2] << 16);
				o.z = (px[2] >> 16) | (px[3] << 8);
				reinterpret_cast<uint3 *>(P.out)[q] = o;
			} else {
				reinterpret_cast<uint4 *>(P.out)[q] =
				    make_uint4(word4(P.format, px[0]), word4(P.format, px[1]), word4(P.format, px[2]), word4(P.format, px[3]));
			}
		}
		if (blockIdx.x == 0 && threadIdx.x < (P.n_px & 3u)) {
			const uint32_t p = 4u * n_quads + threadIdx.x;
			const size_t p3 = 3ull * p;
			const uint32_t b = display_px(P, s, frame, p % W, p / W, P.rgb[p3], P.rgb[p3 + 1], P.rgb[p3 + 2]);
			if (rgb8) {
				uint8_t *o = static_cast<uint8_t *>(P.out) + p3;
				o[0] = (uint8_t)b;
				o[1] = (uint8_t)(b >> 8);
				o[2] = (uint8_t)(b >> 16);
			} else {
				reinterpret_cast<uint32_t *>(P.out)[p] = word4(P.format, b);
			}
		}
	} else {
		for (uint32_t p = gid; p < P.n_px; p += stride) {
			const size_t p3 = 3ull * p;
			const uint32_t b = display_px(P, s, frame, p % W, p / W, P.rgb[p3], P.rgb[p3 + 1], P.rgb[p3 + 2]);
			uint8_t *o = static_cast<uint8_t *>(P.out) + (rgb8 ? p3 : 4ull * p);
			const uint32_t w = rgb8 ? b : word4(P.format, b);
			o[0] = (uint8_t)w;
			o[1] = (uint8_t)(w >> 8);
			o[2] = (uint8_t)(w >> 16);
			if (!rgb8)
				o[3] = (uint8_t)(w >> 24);
		}
	}
}

hipError_t launch_display(hipStream_t stream, const DevDisplayParams &P)
{
	const uint32_t rows = display_hist_blocks(P.n_px);
	const bool in16 = (reinterpret_cast<uintptr_t>(P.rgb) & 15u) == 0u;
	if (in16)
		hipLaunchKernelGGL(display_histogram<true>, dim3(rows), dim3(256), 0, stream, P);
	else
		hipLaunchKernelGGL(display_histogram<false>, dim3(rows), dim3(256), 0, stream, P);
	hipLaunchKernelGGL(display_exposure, dim3(1), dim3(1024), 0, stream, P, rows);
	const uintptr_t o = reinterpret_cast<uintptr_t>(P.out);
	const bool out_aligned = P.format == RT_PIXEL_RGB8 ? (o & 3u) == 0u : (o & 15u) == 0u;
	if (in16 && out_aligned) {
		const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((P.n_px / 4u + 255u) / 256u, 8192u));
		hipLaunchKernelGGL(display_map<true>, dim3(blocks), dim3(256), 0, stream, P);
	} else {
		const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((P.n_px + 255u) / 256u, 16384u));
		hipLaunchKernelGGL(display_map<false>, dim3(blocks), dim3(256), 0, stream, P);
	}
	return hipGetLastError();
}

} // namespace rt
