// rt_temporal.hip -- temporal accumulation with camera reprojection (rt_denoise_temporal, include/rt_hip.h): the temporal half of
// SVGF in front of the A-Trous filter of rt_denoise.hip.  The arithmetic is defined in the header; tests/temporal_checker.py
// restates the per-pixel stage in numpy float32 bit for bit.
//
// Launch sequence (launch_temporal), on one stream:
//   temporal_reproject        one lane per pixel: what denoise_prepass_kernel<1> writes -- plane1 = (e0, lum(e0)) or the invalid mark
//                             (0, 0, 0, NaN), the guide (n^, z) -- with the guide going to H1 of the history written; then the
//                             reprojection into the history read (four bilinear taps through L1 / L2), the motion, H2 = (m1, m2),
//                             and (e, n) stashed in H0 until the feedback overwrites e
//   denoise_variance_kernel   the denoiser's own 5 x 5 spatial estimate, plane1 -> plane0 = (e0, Var)
//   temporal_resolve          plane0 = (e, Var), Var from the moments where n >= 4
//   denoise_iteration_kernel  iteration 0 (never the last: its output must reach the history), plane0 -> plane1
//   temporal_feedback         H0.rgb = e_1 (plane1); with one iteration it also remodulates into out (e_1 * d, the rounding of the
//                             last iteration's sr / sw * d)
//   denoise_iteration_kernel  iterations 1 .. N-1, the last one writing out
// The denoiser kernels are launched through rt_denoise.hip's helpers; this file instantiates none of them.
#include "rt_temporal.h"
#include "rt_post_common.h"

namespace rt {

namespace {

struct V {
	float x, y, z;
};
__device__ inline V vld(const float *a) { return V{a[0], a[1], a[2]}; }
__device__ inline V vadd(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline V vsub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V vmul(V a, float s) { return V{a.x * s, a.y * s, a.z * s}; }
__device__ inline V vdiv(V a, float s) { return V{a.x / s, a.y / s, a.z / s}; }
__device__ inline float vdot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; } // (a.x*b.x + a.y*b.y) + a.z*b.z, no fma
__device__ inline V vcross(V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

} // namespace

__global__ __launch_bounds__(256) void temporal_reproject(const DevTemporalParams P, float4 *__restrict__ plane1, uint32_t tiles_x)
{
	const uint32_t W = P.width, H = P.height, n_px = W * H;
	const float fw = (float)(W - 1u), fh = (float)(H - 1u);
	{ // one 16 x 16 tile per workgroup (no grid-stride loop: nothing uniform has to stay live across tiles)
		uint32_t x, y;
		tile_pixel(blockIdx.x, tiles_x, x, y);
		if (x >= W || y >= H)
			return;
		const uint32_t p = y * W + x;
		const size_t p3 = 3ull * p;
		// ---- the prepass of rt_denoise (denoise_prepass_kernel<1>)
		float e0[3], d[3] = {1.0f, 1.0f, 1.0f};
		if (P.albedo)
			for (int i = 0; i < 3; ++i)
				d[i] = fmaxf(P.albedo[p3 + i], 1e-3f);
		bool valid = true;
		for (int i = 0; i < 3; ++i) {
			const float c = P.color[p3 + i];
			valid = valid && __builtin_isfinite(c);
			e0[i] = c / d[i];
		}
		const float l = lum(e0[0], e0[1], e0[2]);
		valid = valid && __builtin_isfinite(l);
		plane1[p] = valid ? make_float4(e0[0], e0[1], e0[2], l) : make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf(""));
		float4 g = make_float4(0.0f, 0.0f, 0.0f, P.depth[p]);
		if (P.normal) {
			const float nx = P.normal[p3], ny = P.normal[p3 + 1], nz = P.normal[p3 + 2];
			const float len = sqrtf(nx * nx + ny * ny + nz * nz);
			if (len != 0.0f) {
				g.x = nx / len;
				g.y = ny / len;
				g.z = nz / len;
			}
		}
		P.hist_out[n_px + p] = g;

		// ---- reprojection into the previous frame
		float mx = __builtin_nanf(""), my = __builtin_nanf("");
		float e[3] = {e0[0], e0[1], e0[2]}, n = 1.0f, m1 = l, m2 = l * l;
		const float z = g.w;
		const bool hit = z > 0.0f && __builtin_isfinite(z), miss = z == 0.0f;
		if (P.hist_in && (hit || miss)) {
			const V o = vld(P.cam), ll = vld(P.cam + 3), h = vld(P.cam + 6), vv = vld(P.cam + 9);
			const V o2 = vld(P.prev), ll2 = vld(P.prev + 3), h2 = vld(P.prev + 6), v2 = vld(P.prev + 9);
			const float xc = (float)x + 0.5f, yc = (float)y + 0.5f;
			const float u = xc / fw, v = 1.0f - yc / fh;
			const V D = vsub(vadd(vadd(ll, vmul(h, u)), vmul(vv, v)), o);
			const V dh = vdiv(D, sqrtf(vdot(D, D)));
			const V R = hit ? vsub(vadd(o, vmul(dh, z)), o2) : dh;
			const V L = vsub(ll2, o2), chv = vcross(h2, v2);
			const float det = vdot(L, chv);
			const float s = vdot(R, chv) / det, al = vdot(L, vcross(R, v2)) / det, be = vdot(L, vcross(h2, R)) / det;
			if (det != 0.0f && s > 0.0f && __builtin_isfinite(s) && __builtin_isfinite(al) && __builtin_isfinite(be)) {
				const float X = (al / s) * fw, Y = (1.0f - be / s) * fh;
				mx = X - xc;
				my = Y - yc;
				if (valid) {
					const float fx = X - 0.5f, fy = Y - 0.5f;
					const float i0 = floorf(fx), j0 = floorf(fy);
					const float ax = fx - i0, ay = fy - j0, bx = 1.0f - ax, by = 1.0f - ay;
					const float dist = hit ? sqrtf(vdot(R, R)) : 0.0f;
					const float ztol = P.depth_tol * dist;
					const bool np0 = g.x == 0.0f && g.y == 0.0f && g.z == 0.0f;
					float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f, nmax = 0.0f;
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const float ti = (k & 1) ? i0 + 1.0f : i0, tj = (k & 2) ? j0 + 1.0f : j0;
						const float w = ((k & 1) ? ax : bx) * ((k & 2) ? ay : by);
						if (!(ti >= 0.0f && ti <= fw && tj >= 0.0f && tj <= fh && w >= 1.0f / 64.0f))
							continue;
						const uint32_t q = (uint32_t)tj * W + (uint32_t)ti;
						const float4 hq0 = P.hist_in[q];
						if (!(hq0.w >= 1.0f))
							continue;
						const float4 hq1 = P.hist_in[n_px + q];
						if (hit ? !(hq1.w > 0.0f && fabsf(hq1.w - dist) <= ztol) : !(hq1.w == 0.0f))
							continue;
						if (P.normal && !np0 && !(hq1.x == 0.0f && hq1.y == 0.0f && hq1.z == 0.0f) &&
						    !(g.x * hq1.x + g.y * hq1.y + g.z * hq1.z >= P.normal_tol))
							continue;
						const float4 hq2 = P.hist_in[2ull * n_px + q];
						sw = sw + w;
						sr = sr + w * hq0.x;
						sg = sg + w * hq0.y;
						sb = sb + w * hq0.z;
						s1 = s1 + w * hq2.x;
						s2 = s2 + w * hq2.y;
						nmax = fmaxf(nmax, hq0.w);
					}
					if (sw > 0.0f) {
						const float ep[3] = {sr / sw, sg / sw, sb / sw}, m1p = s1 / sw, m2p = s2 / sw;
						n = fminf(nmax + 1.0f, P.max_history);
						const float ac = fmaxf(P.alpha_c, 1.0f / n), am = fmaxf(P.alpha_m, 1.0f / n);
						for (int i = 0; i < 3; ++i)
							e[i] = ep[i] + ac * (e0[i] - ep[i]);
						m1 = m1p + am * (l - m1p);
						m2 = m2p + am * (l * l - m2p);
					}
				}
			}
		}
		if (P.motion) {
			P.motion[2ull * p] = mx;
			P.motion[2ull * p + 1] = my;
		}
		P.hist_out[p] = valid ? make_float4(e[0], e[1], e[2], n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		P.hist_out[2ull * n_px + p] = valid ? make_float4(m1, m2, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	}
}

// plane0 = (e, Var) for the filter: the moments' variance where n >= 4, the spatial estimate (already in plane0) elsewhere
__global__ __launch_bounds__(256) void temporal_resolve(const DevTemporalParams P, float4 *__restrict__ plane0)
{
	const uint32_t n_px = P.width * P.height;
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n_px; p += gridDim.x * 256u) {
		const float spatial = plane0[p].w;
		if (__builtin_isnan(spatial)) // invalid: keeps the mark
			continue;
		const float4 h0 = P.hist_out[p];
		float var = spatial;
		if (h0.w >= 4.0f) {
			const float4 h2 = P.hist_out[2ull * n_px + p];
			var = fmaxf(0.0f, h2.y - h2.x * h2.x);
		}
		plane0[p] = make_float4(h0.x, h0.y, h0.z, var);
	}
}

// H0.rgb = e_1 (iteration 0's output, plane1); with one iteration, out = e_1 * d (valid) or c (invalid) as well
__global__ __launch_bounds__(256) void temporal_feedback(const DevTemporalParams P, const float4 *__restrict__ plane1,
                                                         float *__restrict__ out)
{
	const uint32_t n_px = P.width * P.height;
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n_px; p += gridDim.x * 256u) {
		const float4 e1 = plane1[p];
		const float n = P.hist_out[p].w;
		P.hist_out[p] = make_float4(e1.x, e1.y, e1.z, n);
		if (out) {
			const size_t p3 = 3ull * p;
			if (__builtin_isnan(e1.w)) {
				for (int i = 0; i < 3; ++i)
					out[p3 + i] = P.color[p3 + i];
			} else {
				float d[3] = {1.0f, 1.0f, 1.0f};
				if (P.albedo)
					for (int i = 0; i < 3; ++i)
						d[i] = fmaxf(P.albedo[p3 + i], 1e-3f);
				out[p3] = e1.x * d[0];
				out[p3 + 1] = e1.y * d[1];
				out[p3 + 2] = e1.z * d[2];
			}
		}
	}
}

hipError_t launch_temporal(hipStream_t stream, const DevTemporalParams &T, const DevDenoiseParams &D)
{
	const uint32_t n = T.width * T.height;
	const uint32_t tiles_x = (T.width + 15u) / 16u, n_tiles = tiles_x * ((T.height + 15u) / 16u);
	const dim3 px_blocks(std::min<uint32_t>((n + 255u) / 256u, kMaxBlocks));
	hipLaunchKernelGGL(temporal_reproject, dim3(n_tiles), dim3(256), 0, stream, T, D.plane1, tiles_x);
	launch_denoise_variance(stream, D);
	hipLaunchKernelGGL(temporal_resolve, px_blocks, dim3(256), 0, stream, T, D.plane0);
	// iteration 0 always as a non-last iteration: with N == 1 the parameter block says N = 2 for it, and the feedback remodulates
	DevDenoiseParams D0 = D;
	if (D0.iterations == 1u)
		D0.iterations = 2u;
	launch_denoise_iteration(stream, D0, 0u, D.plane0, D.plane1);
	hipLaunchKernelGGL(temporal_feedback, px_blocks, dim3(256), 0, stream, T, D.plane1, D.iterations == 1u ? D.out : nullptr);
	float4 *src = D.plane1, *dst = D.plane0;
	for (uint32_t i = 1; i < D.iterations; ++i) {
		launch_denoise_iteration(stream, D, i, src, dst);
		std::swap(src, dst);
	}
	return hipGetLastError();
}

} // namespace rt
