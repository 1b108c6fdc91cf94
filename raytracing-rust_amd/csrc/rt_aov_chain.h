// rt_aov_chain.h -- launch interface of the specular-chain AOV kernel (rt_aov_chain.hip), shared with rt_api_post.cpp.
#pragma once

#include "rt_aov.h"

namespace rt {

constexpr uint32_t kAovBounces = 64u;    // the `bounces` channel of rt_aov_chain_buffers (after the kAov* bits of rt_aov.h)
constexpr uint32_t kAovChainMaxChain = 64u; // largest max_chain (include/rt_hip.h rt_aov_chain_opts)

struct DevAovChainParams {
	DevAovParams A;     // what the first-hit pass takes (mask: kAov* | kAovBounces)
	uint32_t max_chain; // followed hits per pass at most
	float fuzz_limit;   // a Reflect is followed when its fuzz <= this
	float *bounces;
};

hipError_t launch_aov_chain(bool prune, hipStream_t stream, const DevScene &S, const DevAovChainParams &P);

} // namespace rt
