// rt_denoise.h -- launch interface of the A-Trous denoiser kernels (rt_denoise.hip), shared with rt_api.cpp.
#pragma once

#include <stdint.h>
#include <hip/hip_runtime.h>

namespace rt {

// the workspace: three float4 planes of w*h -- (e, Var) twice (ping-pong) and (n^, z)
constexpr uint64_t kDenoisePlaneBytes = 16;
constexpr uint64_t kDenoiseWorkspaceBytesPerPixel = 3 * kDenoisePlaneBytes;

struct DevDenoiseParams {
	uint32_t width, height;
	uint32_t iterations;
	float sigma_l, sigma_n, sigma_z;
	const float *color;    // c (rt_render_denoised: the noisy mean the prepass writes)
	const float *albedo, *normal, *depth, *variance; // NULL = not given
	const float *half_a, *half_b; // rt_render_denoised: the two half renders (prepass then writes `color`)
	float *noisy;          // rt_render_denoised: (A + B) * 0.5f, read back as `color` by the last iteration
	float4 *plane0, *plane1, *guide;
	float *out;
};

// prepass (one or two launches) + one launch per iteration, all on `stream`; no allocation, no synchronisation
hipError_t launch_denoise(hipStream_t stream, const DevDenoiseParams &P);

// the parts rt_temporal.hip reuses: the 5 x 5 spatial variance (plane1 -> plane0) and iteration i (step 2^i; the last one,
// i + 1 == P.iterations, remodulates into P.out and ignores dst)
void launch_denoise_variance(hipStream_t stream, const DevDenoiseParams &P);
void launch_denoise_iteration(hipStream_t stream, const DevDenoiseParams &P, uint32_t i, const float4 *src, float4 *dst);

} // namespace rt
