// rt_display.h -- launch interface of the display stage kernels (rt_display.hip), shared with rt_api.cpp.
#pragma once

#include <stdint.h>
#include <hip/hip_runtime.h>

#include "../../include/rt_hip.h"

namespace rt {

constexpr uint32_t kDisplayBins = 256;
constexpr uint32_t kDisplayMaxHistBlocks = 256; // the histogram grid: at most this many workgroups, grid-stride beyond
constexpr uint32_t kDisplayPixelsPerHistBlock = 2048;
// the workspace: a 16-byte block the exposure kernel leaves for the map kernel (2^ev, the dither frame), then one row of 256
// uint32 partial counts per histogram workgroup
constexpr uint64_t kDisplayParamBytes = 16;

inline uint32_t display_hist_blocks(uint64_t n_px)
{
	const uint64_t b = (n_px + kDisplayPixelsPerHistBlock - 1) / kDisplayPixelsPerHistBlock;
	return (uint32_t)(b < 1 ? 1 : (b > kDisplayMaxHistBlocks ? kDisplayMaxHistBlocks : b));
}
inline uint64_t display_workspace_bytes(uint64_t n_px)
{
	return kDisplayParamBytes + (uint64_t)display_hist_blocks(n_px) * kDisplayBins * 4;
}

struct DevDisplayParams {
	uint32_t n_px, width;
	int32_t mode, tonemap, transfer, quantiser, format;
	float exposure_ev, key_ev, meter_low, meter_high, ev_min, ev_max, adaptation;
	float white2;    // white * white
	float hable_fw;  // the Hable curve at `white`, f(w), computed on the host with the same arithmetic
	float inv_gamma; // 1.0f / gamma
	uint32_t seed_lo, seed_hi;
	const float *rgb;
	rt_display_state *state; // NULL = no adaptation, dither frame 0
	char *ws;
	void *out;
	uint32_t *histogram; // NULL = not written
};

// the Hable (Uncharted 2) curve before the white-point division; shared by the host (f(w)) and the map kernel
__host__ __device__ inline float display_hable(float x)
{
	const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
	const float CB = C * B, DE = D * E, DF = D * F, EF = E / F;
	return (x * (A * x + CB) + DE) / (x * (A * x + B) + DF) - EF;
}

// histogram, exposure, map; all on `stream`, no allocation, no synchronisation
hipError_t launch_display(hipStream_t stream, const DevDisplayParams &P);

} // namespace rt
