// rt_render.h -- what rt_render.hip exports to rt_api.cpp: the sizes a launch is planned from, the occupancy query, the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_types.h"
#include "rt_sky_tiles.h"

namespace rt {
// ---- what plan_render_launch sizes a launch from (feature_set: 0 spheres-only, 1 simple, 2 full, 3 FeatPair) ----
size_t render_lds_bytes(const DevScene &S, bool sky_lds, bool scene_lds, uint32_t waves_per_block, uint32_t stack_cap);
uint32_t render_waves_per_simd(int feature_set, bool fine);
uint32_t render_block_threads(int feature_set, bool fine, bool xchg = false);
uint32_t render_max_block_threads(int feature_set, bool fine, bool xchg);
hipError_t render_occupancy(int method, bool prune, bool fine, bool sky_lds, int feature_set, size_t lds_bytes, int *blocks_per_cu, bool xchg,
                            uint32_t block_threads = 0);
// RT_TUNE_EXCHANGE: where it is built, and the LDS of its pools
bool render_exchange_available(int method, bool prune, bool fine, int feature_set);
size_t render_exchange_lds_bytes(uint32_t slots);
uint32_t render_exchange_max_slots();
size_t render_exchange_fine_lds_bytes(uint32_t waves_per_block);

// ---- a render: reset, the persistent kernel, the fold of a sample_split's chunks ----
hipError_t launch_reset(hipStream_t stream, uint32_t *work_counter, unsigned long long *rays_shot, float *out, size_t n_out_floats);
hipError_t launch_render(int method, bool prune, bool fine, bool sky_lds, int feature_set, uint32_t n_blocks, size_t lds_bytes, hipStream_t stream,
                         const DevScene &S, const DevCamera &cam, const DevRenderParams &P, float *out,
                         unsigned long long *rays_shot, uint32_t *work_counter, uint32_t *stack_ovf, bool xchg, const DevPairScene *pair,
                         const DevPairPrimary *primary, uint32_t block_threads, const DevSkyTiles &sky_tiles, const DevSkyCell &sky_cell);
hipError_t launch_combine(hipStream_t stream, const DevRenderParams &P, const float *partial, float *out);
// ---- multi-device scenes, output ----
hipError_t launch_scatter_shard(hipStream_t stream, const DevRenderParams &P, const float *shard, float *frame);
hipError_t launch_sum_u64(hipStream_t stream, const unsigned long long *parts, uint32_t n, unsigned long long *out);
hipError_t launch_quantise(hipStream_t stream, const float *rgb, size_t n_values, float inv_gamma, uint8_t *out);
} // namespace rt
