// rt_dof.hip -- the depth-of-field stage (rt_dof, include/rt_hip.h): a W x H RGB float frame and its depth plane to a W x H frame in
// which every pixel is spread over the disc of its circle of confusion, gathered, a blurred background kept off a sharper
// foreground.  The arithmetic is defined in the header; tests/dof_checker.py restates it in numpy bit for bit.
//
// Launch sequence (launch_dof), on one stream:
//   dof_coc_kernel     one lane per pixel, grid-stride: depth (and the camera, for planar depth) -> (radius, depth key) in the
//                      workspace, and the signed radius plane when it is asked for
//   dof_gather_kernel  a 256-thread workgroup makes a 32 x 8 tile of the output: it stages the tile and a max_radius halo of
//                      (r, g, b, radius, depth key) in LDS -- indices clamped to the image, the radius of a pixel off the frame
//                      or with a non-finite channel set to 0, which is a tap that covers nothing -- reduces the largest staged
//                      radius over the workgroup and runs the tap loops as far as that radius reaches: a tap beyond it has zero
//                      cover, so the bytes are those of the full loops (the header allows exactly this).  A tile wholly in focus
//                      costs one tap per pixel.  The four sums live in registers; sqrtf(dx*dx + dy*dy) comes from a 17 x 17 table
//                      the workgroup fills with sqrtf itself.  Capped grid, grid-stride over the tiles.
// LDS: 5 planes of 64 x 40 floats (the footprint at max_radius 16) = 51 200 bytes, the table 1 156, the four wave maxima 16:
// 52 372 bytes, three workgroups (twelve waves) per CU of 160 KB.
#include <algorithm>
#include <cfloat>

#include "rt_dof.h"
#include "rt_post_common.h"

namespace rt {

namespace {

constexpr uint32_t kTab = kDofMaxRadius + 1u; // side of the distance table

struct V {
	float x, y, z;
};
__device__ inline V vld(const float *p) { return V{p[0], p[1], p[2]}; }
__device__ inline float vdot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; } // (a.x*b.x + a.y*b.y) + a.z*b.z, no fma
// ((ll + hz*u) + vt*v) - o per component, then / sqrtf(dot): the direction of the camera ray through (u, v), normalised
__device__ inline V ray_dir(V o, V ll, V hz, V vt, float u, float v)
{
	const V d = {((ll.x + hz.x * u) + vt.x * v) - o.x, ((ll.y + hz.y * u) + vt.y * v) - o.y, ((ll.z + hz.z * u) + vt.z * v) - o.z};
	const float m = sqrtf(vdot(d, d));
	return V{d.x / m, d.y / m, d.z / m};
}

} // namespace

__global__ __launch_bounds__(256) void dof_coc_kernel(const DevDofParams P)
{
	const uint32_t n = P.width * P.height, stride = gridDim.x * 256u;
	const V o = vld(P.cam), ll = vld(P.cam + 3), hz = vld(P.cam + 6), vt = vld(P.cam + 9);
	const V fwd = P.planar ? ray_dir(o, ll, hz, vt, 0.5f, 0.5f) : V{0.0f, 0.0f, 0.0f};
	const float w1 = (float)(P.width - 1u), h1 = (float)(P.height - 1u), cap = (float)P.max_radius;
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += stride) {
		const float t = P.depth[p];
		float z = t;
		if (P.planar) {
			const uint32_t y = p / P.width, x = p - y * P.width;
			const float u = (float)x / w1, v = 1.0f - (float)y / h1;
			z = t * vdot(ray_dir(o, ll, hz, vt, u, v), fwd);
		}
		const bool at_infinity = !(__builtin_isfinite(t) && t > 0.0f && z > 0.0f);
		const float k = at_infinity ? 1.0f : fminf(fabsf(z - P.focus_distance) / z, FLT_MAX);
		const float r = fmaxf(0.5f, fminf(P.blur_scale * k, cap));
		P.ws[p] = make_float2(r, at_infinity ? __builtin_inff() : z);
		if (P.coc)
			P.coc[p] = (!at_infinity && z < P.focus_distance) ? -r : r;
	}
}

__global__ __launch_bounds__(256) void dof_gather_kernel(const DevDofParams P, uint32_t tiles_x, uint32_t n_tiles)
{
	__shared__ float s_rgb[3][kDofFootPixels];
	__shared__ float2 s_rk[kDofFootPixels]; // (radius, depth key)
	__shared__ float s_d[kTab * kTab];      // sqrtf(a*a + b*b) at [a][b]
	__shared__ float s_wave_max[4];
	const uint32_t t = threadIdx.x, lx = t & (kDofTileW - 1u), ly = t / kDofTileW;
	const int R = (int)P.max_radius;
	const uint32_t FW = kDofTileW + 2u * P.max_radius, FH = kDofTileH + 2u * P.max_radius;
	for (uint32_t i = t; i < kTab * kTab; i += 256u) {
		const uint32_t a = i / kTab, b = i - a * kTab;
		s_d[i] = sqrtf((float)(a * a + b * b));
	}
	for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
		const uint32_t X0 = tx * kDofTileW, Y0 = ty * kDofTileH;
		// the footprint: local (li, lj) is pixel (X0 - R + li, Y0 - R + lj); lanes run along rows
		float m = 0.0f;
		for (uint32_t i = t; i < FW * FH; i += 256u) {
			const uint32_t lj = i / FW, li = i - lj * FW;
			const long long gx = (long long)X0 - R + li, gy = (long long)Y0 - R + lj;
			const bool inside = gx >= 0 && gx < (long long)P.width && gy >= 0 && gy < (long long)P.height;
			const uint32_t cx = gx < 0 ? 0u : (gx >= (long long)P.width ? P.width - 1u : (uint32_t)gx);
			const uint32_t cy = gy < 0 ? 0u : (gy >= (long long)P.height ? P.height - 1u : (uint32_t)gy);
			const size_t q = (size_t)cy * P.width + cx;
			const float *px = P.rgb + 3u * q;
			const float r = px[0], g = px[1], b = px[2];
			float2 rk = P.ws[q];
			if (!inside || !finite3(r, g, b))
				rk.x = 0.0f; // a skipped tap: radius 0 covers no other pixel
			s_rgb[0][i] = r;
			s_rgb[1][i] = g;
			s_rgb[2][i] = b;
			s_rk[i] = rk;
			m = fmaxf(m, rk.x);
		}
#pragma unroll
		for (int s = 32; s >= 1; s >>= 1)
			m = fmaxf(m, __shfl_xor(m, s));
		if ((t & 63u) == 0u)
			s_wave_max[t >> 6] = m;
		__syncthreads();
		const float rmax = fmaxf(fmaxf(s_wave_max[0], s_wave_max[1]), fmaxf(s_wave_max[2], s_wave_max[3]));
		// offset n of a tap matters only where n - 0.5 < its radius: the largest such n is ceil(rmax - 0.5) (the difference is exact)
		const int Rb = std::min(R, std::max(0, (int)ceilf(rmax - 0.5f)));
		const uint32_t ci = (ly + (uint32_t)R) * FW + lx + (uint32_t)R;
		const float c0 = s_rgb[0][ci], c1 = s_rgb[1][ci], c2 = s_rgb[2][ci];
		const float2 prk = s_rk[ci];
		const float r_p = prk.x, key_p = prk.y; // (r_p is 0 where this pixel passes through: its sums are not used)
		float sw = -0.0f, s0 = -0.0f, s1 = -0.0f, s2 = -0.0f;
		for (int dy = -Rb; dy <= Rb; ++dy) {
			const int row = (int)ci + dy * (int)FW;
			const float *drow = s_d + (uint32_t)(dy < 0 ? -dy : dy) * kTab;
			for (int dx = -Rb; dx <= Rb; ++dx) {
				const uint32_t qi = (uint32_t)(row + dx);
				const float2 q = s_rk[qi];
				const float d = drow[dx < 0 ? -dx : dx];
				const float re = q.y > key_p ? fminf(q.x, r_p) : q.x;
				const float cover = fminf(fmaxf((re - d) + 0.5f, 0.0f), 1.0f);
				if (cover != 0.0f) {
					const float dm = re + re;
					const float w = cover / (dm * dm);
					sw = sw + w;
					s0 = s0 + w * s_rgb[0][qi];
					s1 = s1 + w * s_rgb[1][qi];
					s2 = s2 + w * s_rgb[2][qi];
				}
			}
		}
		const uint32_t X = X0 + lx, Y = Y0 + ly;
		if (X < P.width && Y < P.height) {
			float *o = P.out + 3u * ((size_t)Y * P.width + X);
			const bool keep = !finite3(c0, c1, c2) || sw == 0.0f;
			o[0] = keep ? c0 : s0 / sw;
			o[1] = keep ? c1 : s1 / sw;
			o[2] = keep ? c2 : s2 / sw;
		}
		__syncthreads(); // the next trip overwrites the footprint and the maxima
	}
}

hipError_t launch_dof(hipStream_t stream, const DevDofParams &P)
{
	const uint64_t n = (uint64_t)P.width * P.height;
	const uint32_t blocks = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>((n + 255u) / 256u, kDofMaxBlocks));
	hipLaunchKernelGGL(dof_coc_kernel, dim3(blocks), dim3(256), 0, stream, P);
	const uint32_t tiles_x = (P.width + kDofTileW - 1u) / kDofTileW, n_tiles = tiles_x * ((P.height + kDofTileH - 1u) / kDofTileH);
	hipLaunchKernelGGL(dof_gather_kernel, dim3(std::min(n_tiles, kDofMaxTiles)), dim3(256), 0, stream, P, tiles_x, n_tiles);
	return hipGetLastError();
}

} // namespace rt
