// rt_temporal.h -- launch interface of the temporal accumulation kernels (rt_temporal.hip), shared with rt_api.cpp.
#pragma once

#include <stdint.h>
#include <hip/hip_runtime.h>

#include "rt_denoise.h"

namespace rt {

// one history buffer: three float4 planes of w*h -- H0 = (e_1.rgb, n), H1 = (n^.xyz, z), H2 = (m1, m2, 0, 0)
constexpr uint64_t kTemporalHistoryBytesPerPixel = 3 * 16;
// the workspace: plane0 and plane1 of the denoiser (the guide plane is H1 of the history written)
constexpr uint64_t kTemporalWorkspaceBytesPerPixel = 2 * kDenoisePlaneBytes;

struct DevTemporalParams {
	uint32_t width, height;
	float cam[12], prev[12]; // rt_camera: origin, lower_left, horizontal, vertical
	float alpha_c, alpha_m, depth_tol, normal_tol, max_history;
	const float *color, *albedo, *normal, *depth;   // albedo / normal NULL = not given
	const float4 *hist_in;                           // H0, H1, H2 one after the other; NULL = no history
	float4 *hist_out;
	float *motion;                                   // NULL = not written
};

// reprojection, the denoiser's variance pass, resolve, the A-Trous iterations with the history feedback after iteration 0; all on
// `stream`, no allocation, no synchronisation.  D is the denoiser's parameter block for the same frame (variance NULL, guide = h1_out).
hipError_t launch_temporal(hipStream_t stream, const DevTemporalParams &T, const DevDenoiseParams &D);

} // namespace rt
