// rt_upscale.h -- launch interface of the AOV-guided upscaling kernel (rt_upscale.hip), shared with rt_api_post.cpp.
#pragma once

#include <stdint.h>
#include <hip/hip_runtime.h>

#include "../../include/rt_hip.h"

namespace rt {

struct DevUpscaleParams {
	uint32_t w, h; // source frame
	uint32_t W, H; // destination frame, W >= w, H >= h
	float sigma_n, depth_tol;
	const float *color;                                // w*h*3
	const float *src_albedo, *src_normal, *src_depth;  // NULL = that guide not used (then NULL at both sizes)
	const float *dst_albedo, *dst_normal, *dst_depth;
	float *out;     // W*H*3
	uint8_t *stage; // W*H, NULL = not written
};

// one kernel on `stream`, no allocation, no workspace, no synchronisation
hipError_t launch_upscale(hipStream_t stream, const DevUpscaleParams &P);

} // namespace rt
