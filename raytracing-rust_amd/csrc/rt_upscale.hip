// rt_upscale.hip -- AOV-guided upscaling (rt_upscale, include/rt_hip.h): joint bilateral upsampling (Kopf et al., SIGGRAPH 2007) of
// albedo-demodulated radiance from a w x h frame to a W x H frame, guided by the first-hit albedo, normal and depth at both sizes.
// The arithmetic is defined in the header; tests/upscale_checker.py restates it in numpy float32 bit for bit.
//
// One kernel (stable name for rocprofv3), upscale_kernel<ALBEDO, NORMAL, DEPTH>, templated on the guide set.  A 256-thread workgroup
// takes one 16 x 16 destination tile, wave w its 8 x 8 quadrant (w & 1, w >> 1), one lane per pixel (the denoiser's tiling).  The
// source pixels a tile can tap -- the bilinear footprint plus the ring of the 4 x 4 window, at most 20 x 20 for W >= w, H >= h --
// are demodulated and normalised ONCE into LDS as two float4 each, (e, valid) and (n^, z), with the frame-edge clamp applied while
// filling; every tap is then two 16-byte LDS reads at an unclamped footprint coordinate.  Destination guides are read once per
// lane and the output is written once.  The 4 x 4 stage and the nearest-tap stage are rare (silhouettes): they sit behind one
// branch in rolled loops, so that the four unrolled taps of stage 1 set the register budget.
#include "rt_upscale.h"
#include "rt_post_common.h"

#include "../../include/rt_detmath.h"

namespace rt {

namespace {

constexpr int kFoot = 20; // footprint side: 16 destination pixels span at most 17 values of floorf(fx), plus 1 before and 2 after

// where destination pixel centre x falls in the source frame, minus the half pixel of the tap centres: fx of the header
__device__ inline float src_coord(uint32_t x, float dst_m1, float src_m1) { return (((float)x + 0.5f) / dst_m1) * src_m1 - 0.5f; }

struct DstPixel {
	float nx, ny, nz; // n^(p)
	bool n0;          // n^(p) == 0
	float z, ztol;    // z(p), depth_tolerance * z(p)
};

// g of a tap with guide (n^_s, z_s): w_n * w_z
template <bool NORMAL, bool DEPTH> __device__ inline float guide_weight(const DstPixel &p, const float4 gq, float sigma_n)
{
	float wn = 1.0f, wz = 1.0f;
	if (NORMAL) {
		const bool q0 = gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f;
		if (!(p.n0 || q0))
			wn = rt_powf(fmaxf(0.0f, (p.nx * gq.x + p.ny * gq.y) + p.nz * gq.z), sigma_n);
	}
	if (DEPTH) {
		if (p.z == 0.0f || gq.w == 0.0f) {
			wz = (p.z == 0.0f && gq.w == 0.0f) ? 1.0f : 0.0f;
		} else {
			const float t = fabsf(p.z - gq.w) / p.ztol;
			wz = t < 1.0f ? (1.0f - t) * (1.0f - t) : 0.0f;
		}
	}
	return wn * wz;
}

__device__ inline float tent(float d) { return fmaxf(0.0f, 1.0f - fabsf(d) * 0.4f); }

} // namespace

template <bool ALBEDO, bool NORMAL, bool DEPTH>
__global__ __launch_bounds__(256) void upscale_kernel(const DevUpscaleParams P, uint32_t tiles_x)
{
	__shared__ float4 s_e[kFoot * kFoot]; // (e.rgb, 1) of a valid source pixel, (0, 0, 0, 0) of an invalid one
	__shared__ float4 s_g[kFoot * kFoot]; // (n^.xyz, z)
	const uint32_t w = P.w, h = P.h, W = P.W, H = P.H;
	const float src_mx = (float)(w - 1u), src_my = (float)(h - 1u), dst_mx = (float)(W - 1u), dst_my = (float)(H - 1u);
	const uint32_t tx0 = (blockIdx.x % tiles_x) * 16u, ty0 = (blockIdx.x / tiles_x) * 16u;

	// ---- the tile's source footprint [ilo, ilo + nx) x [jlo, jlo + ny) in unclamped source coordinates (workgroup-uniform)
	const int ilo = (int)floorf(src_coord(tx0, dst_mx, src_mx)) - 1, jlo = (int)floorf(src_coord(ty0, dst_my, src_my)) - 1;
	const int ihi = (int)floorf(src_coord(min(tx0 + 15u, W - 1u), dst_mx, src_mx)) + 2;
	const int jhi = (int)floorf(src_coord(min(ty0 + 15u, H - 1u), dst_my, src_my)) + 2;
	const int nx = min(ihi - ilo + 1, kFoot), ny = min(jhi - jlo + 1, kFoot);
	for (int k = (int)threadIdx.x; k < nx * ny; k += 256) {
		const int fi = k % nx, fj = k / nx;
		const uint32_t si = (uint32_t)min(max(ilo + fi, 0), (int)w - 1), sj = (uint32_t)min(max(jlo + fj, 0), (int)h - 1);
		const size_t q = (size_t)sj * w + si, q3 = 3u * q;
		float d[3] = {1.0f, 1.0f, 1.0f}, c[3], e[3];
		if (ALBEDO)
			for (int i = 0; i < 3; ++i)
				d[i] = fmaxf(P.src_albedo[q3 + i], 1e-3f);
		for (int i = 0; i < 3; ++i) {
			c[i] = P.color[q3 + i];
			e[i] = c[i] / d[i];
		}
		const bool valid = __builtin_isfinite(c[0]) && __builtin_isfinite(c[1]) && __builtin_isfinite(c[2]) &&
		                   __builtin_isfinite(lum(e[0], e[1], e[2]));
		float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (NORMAL) {
			const float nx_ = P.src_normal[q3], ny_ = P.src_normal[q3 + 1], nz_ = P.src_normal[q3 + 2];
			const float len = sqrtf(nx_ * nx_ + ny_ * ny_ + nz_ * nz_);
			if (len != 0.0f) {
				g.x = nx_ / len;
				g.y = ny_ / len;
				g.z = nz_ / len;
			}
		}
		if (DEPTH)
			g.w = P.src_depth[q];
		s_e[fj * kFoot + fi] = valid ? make_float4(e[0], e[1], e[2], 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		s_g[fj * kFoot + fi] = g;
	}
	__syncthreads();

	// ---- one destination pixel per lane
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t x = tx0 + (wave & 1u) * 8u + (lane & 7u), y = ty0 + (wave >> 1) * 8u + (lane >> 3);
	if (x >= W || y >= H)
		return;
	const size_t p = (size_t)y * W + x, p3 = 3u * p;
	const float fx = src_coord(x, dst_mx, src_mx), fy = src_coord(y, dst_my, src_my);
	const float i0 = floorf(fx), j0 = floorf(fy);
	const float ax = fx - i0, ay = fy - j0, bx = 1.0f - ax, by = 1.0f - ay;
	// the slot of tap (i0, j0): 1 .. kFoot - 3 by the footprint's construction (the clamp only guards the LDS against frame sizes
	// whose coordinates float arithmetic no longer separates)
	const int li = min(max((int)i0 - ilo, 1), kFoot - 3), lj = min(max((int)j0 - jlo, 1), kFoot - 3);

	DstPixel dp = {0.0f, 0.0f, 0.0f, true, 0.0f, 0.0f};
	if (NORMAL) {
		const float nx_ = P.dst_normal[p3], ny_ = P.dst_normal[p3 + 1], nz_ = P.dst_normal[p3 + 2];
		const float len = sqrtf(nx_ * nx_ + ny_ * ny_ + nz_ * nz_);
		if (len != 0.0f) {
			dp.nx = nx_ / len;
			dp.ny = ny_ / len;
			dp.nz = nz_ / len;
		}
		dp.n0 = dp.nx == 0.0f && dp.ny == 0.0f && dp.nz == 0.0f;
	}
	if (DEPTH) {
		dp.z = P.dst_depth[p];
		dp.ztol = P.depth_tol * dp.z;
	}

	// ---- stage 1: the four bilinear taps
	float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int slot = (lj + (k >> 1)) * kFoot + li + (k & 1);
		const float4 eq = s_e[slot];
		const float b = ((k & 1) ? ax : bx) * ((k & 2) ? ay : by);
		const float g = eq.w != 0.0f ? guide_weight<NORMAL, DEPTH>(dp, s_g[slot], P.sigma_n) : 0.0f;
		const float bg = b * g;
		sw = sw + bg;
		sr = sr + bg * eq.x;
		sg = sg + bg * eq.y;
		sb = sb + bg * eq.z;
	}
	float er, eg, eb;
	uint32_t stage = 1u;
	if (sw >= 1.0f / 16.0f) {
		er = sr / sw;
		eg = sg / sw;
		eb = sb / sw;
	} else {
		// ---- stage 2: the 4 x 4 window under a wide tent, rows outer
		sw = sr = sg = sb = 0.0f;
#pragma unroll 1
		for (int k = 0; k < 16; ++k) {
			const int di = (k & 3) - 1, dj = (k >> 2) - 1;
			const int slot = (lj + dj) * kFoot + li + di;
			const float4 eq = s_e[slot];
			const float g = eq.w != 0.0f ? guide_weight<NORMAL, DEPTH>(dp, s_g[slot], P.sigma_n) : 0.0f;
			const float wt = g * tent((i0 + (float)di) - fx) * tent((j0 + (float)dj) - fy);
			sw = sw + wt;
			sr = sr + wt * eq.x;
			sg = sg + wt * eq.y;
			sb = sb + wt * eq.z;
		}
		if (sw >= 1.0f / 1024.0f) {
			stage = 2u;
			er = sr / sw;
			eg = sg / sw;
			eb = sb / sw;
		} else {
			// ---- stage 3: the valid bilinear tap of the largest weight; stage 0: none
			stage = 0u;
			er = eg = eb = 0.0f;
			float best = 0.0f;
#pragma unroll 1
			for (int k = 0; k < 4; ++k) {
				const float4 eq = s_e[(lj + (k >> 1)) * kFoot + li + (k & 1)];
				const float b = ((k & 1) ? ax : bx) * ((k & 2) ? ay : by);
				if (eq.w != 0.0f && (stage == 0u || b > best)) {
					stage = 3u;
					best = b;
					er = eq.x;
					eg = eq.y;
					eb = eq.z;
				}
			}
		}
	}
	float d[3] = {1.0f, 1.0f, 1.0f};
	if (ALBEDO)
		for (int i = 0; i < 3; ++i)
			d[i] = fmaxf(P.dst_albedo[p3 + i], 1e-3f);
	P.out[p3] = er * d[0];
	P.out[p3 + 1] = eg * d[1];
	P.out[p3 + 2] = eb * d[2];
	if (P.stage)
		P.stage[p] = (uint8_t)stage;
}

hipError_t launch_upscale(hipStream_t stream, const DevUpscaleParams &P)
{
	const uint32_t tiles_x = (P.W + 15u) / 16u, n_tiles = tiles_x * ((P.H + 15u) / 16u);
	const dim3 grid(n_tiles), block(256);
	const int set = (P.src_albedo ? 1 : 0) | (P.src_normal ? 2 : 0) | (P.src_depth ? 4 : 0);
	switch (set) {
	case 0: hipLaunchKernelGGL((upscale_kernel<false, false, false>), grid, block, 0, stream, P, tiles_x); break;
	case 1: hipLaunchKernelGGL((upscale_kernel<true, false, false>), grid, block, 0, stream, P, tiles_x); break;
	case 2: hipLaunchKernelGGL((upscale_kernel<false, true, false>), grid, block, 0, stream, P, tiles_x); break;
	case 3: hipLaunchKernelGGL((upscale_kernel<true, true, false>), grid, block, 0, stream, P, tiles_x); break;
	case 4: hipLaunchKernelGGL((upscale_kernel<false, false, true>), grid, block, 0, stream, P, tiles_x); break;
	case 5: hipLaunchKernelGGL((upscale_kernel<true, false, true>), grid, block, 0, stream, P, tiles_x); break;
	case 6: hipLaunchKernelGGL((upscale_kernel<false, true, true>), grid, block, 0, stream, P, tiles_x); break;
	default: hipLaunchKernelGGL((upscale_kernel<true, true, true>), grid, block, 0, stream, P, tiles_x); break;
	}
	return hipGetLastError();
}

} // namespace rt
