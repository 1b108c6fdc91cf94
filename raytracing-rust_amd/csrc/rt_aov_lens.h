// rt_aov_lens.h -- launch interface of the lens-camera AOV kernel (rt_aov_lens.hip), shared with rt_api_lens.cpp.
#pragma once

#include "rt_aov_chain.h"
#include "rt_lens.h"

namespace rt {

// what the chain pass takes (C.A.cam: rt_lens_camera.pinhole), then the rest of rt_lens_camera as DevLensParams holds it
struct DevAovLensParams {
	DevAovChainParams C;
	float right[3], up[3], forward[3]; // SimpleCamera::new's u, v and -w
	float lens_radius;                 // PERSPECTIVE: 0 = no lens draw and no lens arithmetic
	float fisheye_half_angle;          // FISHEYE
	int32_t projection;                // rt_projection (kProj*, rt_lens.h), checked by the host
};

hipError_t launch_aov_lens(bool prune, hipStream_t stream, const DevScene &S, const DevAovLensParams &P);

} // namespace rt
