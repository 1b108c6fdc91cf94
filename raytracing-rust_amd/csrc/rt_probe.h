// rt_probe.h -- launch interface of the light probes (rt_probe.hip), shared with rt_api_probe.cpp.
#pragma once

#include "rt_types.h"

namespace rt {

// the 27 sums of a (probe, chunk) slot: 9 basis functions x RGB
constexpr uint32_t kProbeTerms = 27;

// rt_probe_opts as the kernels take it.  A SLOT is (probe, chunk): slot = probe * split + chunk.  `records` is the caller's
// workspace, laid out [term][slot] (term = 3 j + channel): the lanes of a wave hold neighbouring slots, so each of the 27
// accesses of a fold is a run of neighbouring words
struct DevProbeParams {
	const float *positions;        // [n_probes][3]
	float *records;                // [27][n_slots]
	float *out;                    // [n_probes][9][3]
	unsigned long long *rays_shot; // or null; zeroed ahead of the launch (launch_probe)
	uint32_t n_probes, samples, split;
	uint32_t n_slots;              // n_probes * split, below 2^31 (the host refuses more)
	uint32_t seed_lo, seed_hi, sample_begin_lo, sample_begin_hi;
	uint32_t max_depth, rr_threshold;
	uint32_t convolve;
};

struct DevProbeEvalParams {
	const float *coeffs;         // [n_probes][9][3]
	const uint32_t *probe_index; // [m] or null: element i reads probe i
	const float *normals;        // [m][3]
	float *out;                  // [m][3]
	uint64_t n_probes, m;
};

// waves per SIMD probe_kernel is compiled for (as lens_kernel)
constexpr uint32_t kProbeWaves = 4;
// dynamic LDS of a workgroup behind its four_wave_stack_lds_bytes: eight words a lane (rt_probe.hip)
constexpr uint32_t kProbeRecordWords = 8;
constexpr size_t kProbeRecordLdsBytes = kProbeRecordWords * 256u * sizeof(uint32_t);

inline uint64_t probe_workspace_bytes(uint64_t n_probes, uint32_t split) { return (uint64_t)kProbeTerms * sizeof(float) * n_probes * split; }

// the counter zeroed by a kernel, `groups` 256-thread workgroups of probe_kernel, then the combine of the chunk records
hipError_t launch_probe(int method, bool prune, hipStream_t stream, const DevScene &S, const DevProbeParams &P, uint32_t groups);
hipError_t launch_probe_eval(hipStream_t stream, const DevProbeEvalParams &P);

} // namespace rt
